"""ctypes binding of libkcount_mi355.so (include/kcount_mi355.h, include/kcount_mi355_correct.h, include/kcount_mi355_polish.h,
include/kcount_mi355_break.h).  No fallback of any kind."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

KC_OK = 0
KC_ERR_INVALID_ARG = -1
KC_ERR_CAPACITY = -6
KC_ERR_UNSUPPORTED_K = -2
KC_ERR_BAD_BASE = -7
KC_ERR_STATE = -8
KC_FLAG_TIME_KERNELS = 1
KC_FASTQ_PARTIAL = 1
KC_ADAPTERS_BLASTN_SCORES = 1
KC_TRIM_PAIRED = 1
KC_FLAG_REFERENCE_OWNER = 2
KC_FLAG_SHARD_BUCKETS = 4
KC_FLAG_WIRE_UNITS = 8


class KcError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        L = lib()
        msg = L.kc_error_string(status).decode()
        detail = L.kc_last_error().decode()
        super().__init__("%s: %s (%d)%s" % (where, msg, status, (" -- " + detail) if detail and status in (-3, -4, -5, -6) else ""))


class kc_config(C.Structure):
    _fields_ = [("kmer_len", C.c_int32), ("qual_offset", C.c_int32), ("dmin_thres", C.c_int32), ("device", C.c_int32),
                ("rank_me", C.c_int32), ("rank_n", C.c_int32), ("max_elems", C.c_uint64), ("flags", C.c_uint32),
                ("reserved", C.c_uint32), ("max_kmers_buffered", C.c_uint64)]


class kc_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("num_reads", "num_bases", "raw_kmers", "kmers_inserted", "num_unique", "num_purged",
                                           "total_kmers", "sum_counts", "num_dropped", "capacity", "num_gpu_calls",
                                           "table_bytes")]


class kc_result(C.Structure):
    _fields_ = [("n", C.c_uint64), ("num_longs", C.c_int32), ("reserved", C.c_int32), ("d_keys", C.c_void_p),
                ("d_counts", C.c_void_p), ("d_left", C.c_void_p), ("d_right", C.c_void_p)]


class kc_tuning(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("writers", C.c_uint32), ("p1", C.c_uint32), ("p2", C.c_uint32), ("slots", C.c_uint32),
                ("chunk1", C.c_uint32), ("chunk2", C.c_uint32), ("chain1_max", C.c_uint32), ("chain2_max", C.c_uint32),
                ("arena1", C.c_uint32), ("ovf_capacity", C.c_uint64)]


class kc_kernel_time(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double)]


class kc_synth_params(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("num_genomes", C.c_uint32), ("read_len", C.c_uint32), ("min_genome_len", C.c_uint64),
                ("max_genome_len", C.c_uint64), ("sub_error_rate", C.c_double), ("lowq_rate", C.c_double),
                ("n_rate", C.c_double), ("abundance_sigma", C.c_double)]


class kc_merge_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("pairs", "merged", "ambiguous", "dropped", "overlap_len", "merged_len", "out_reads",
                                           "out_bases")]


class kc_trim_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads", "trimmed", "bases_trimmed", "reads_removed", "alignments", "out_bases")]


class kc_unitig_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("kmers", "unitigs", "singletons", "circular", "bases", "longest")]


class kc_ctg_index_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("contigs", "bases", "windows", "seeds", "repeated")]


class kc_align_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads", "reads_aligned", "windows", "seed_hits", "repeated_hits", "alignments", "perfect")]


class kc_read_aln(C.Structure):
    _fields_ = [("read", C.c_uint32), ("ctg", C.c_uint32), ("cstart", C.c_uint32), ("cstop", C.c_uint32), ("rstart", C.c_uint16),
                ("rstop", C.c_uint16), ("mismatches", C.c_uint16), ("seeds", C.c_uint16), ("orient", C.c_uint8), ("pad", C.c_uint8 * 7)]


KC_ALIGN_MAX_READ_LEN = 1024
KC_ALIGN_KEEP_ALL = 0xFFFFFFFF


class kc_aln_scores(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("match", "mismatch", "gap_open", "gap_ext", "ambiguity")]


class kc_gap_aln(C.Structure):
    _fields_ = [("read", C.c_uint32), ("ctg", C.c_uint32), ("cstart", C.c_uint32), ("cstop", C.c_uint32), ("rstart", C.c_uint16),
                ("rstop", C.c_uint16), ("score", C.c_uint32), ("mismatches", C.c_uint16), ("seeds", C.c_uint16), ("orient", C.c_uint8),
                ("kind", C.c_uint8), ("pad", C.c_uint8 * 2)]


class kc_gap_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("records", "exact", "dp", "none", "cells", "score_sum")]


KC_GAP_MAX_PAD = 1024
KC_GAP_ALWAYS_DP = 1
KC_GAP_EXACT, KC_GAP_DP, KC_GAP_NONE = 0, 1, 2


class kc_ctg_depth(C.Structure):
    _fields_ = [("depth_sum", C.c_uint64)] + [(n, C.c_uint32) for n in ("len", "covered", "min_depth", "max_depth", "alns", "mean")]


class kc_depth_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("records", "none", "filtered", "not_best", "clipped_away", "used", "bases_covered", "depth_sum",
                                          "saturated")]


class kc_pair_rec(C.Structure):
    _fields_ = [("aln0", C.c_uint32), ("aln1", C.c_uint32), ("insert", C.c_uint32), ("cls", C.c_uint8), ("pad", C.c_uint8 * 3)]


class kc_insert_stats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("cls", C.c_uint64 * 7), ("insert_sum", C.c_uint64), ("insert_sq_sum", C.c_uint64),
                ("reads_with_best", C.c_uint64)]


KC_DEPTH_MAX_EDGE = 1024
KC_DEPTH_BEST_ONLY, KC_DEPTH_PER_CONTIG = 1, 2
KC_INSERT_MAX = 65535
KC_PAIR_NONE, KC_PAIR_ONE, KC_PAIR_DIFF_CTG, KC_PAIR_SAME_ORIENT, KC_PAIR_EVERTED, KC_PAIR_TOO_LONG, KC_PAIR_PROPER = range(7)


class kc_lassm_params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("min_mer_len", "max_mer_len", "shift", "max_walk_len", "max_insert", "min_qual", "hi_qual",
                                          "min_viable", "viable_permille", "max_cands", "table_budget_mb", "flags")]


class kc_lassm_end(C.Structure):
    _fields_ = [("cands", C.c_uint32), ("ext_len", C.c_uint32), ("out_pos", C.c_uint32), ("iters", C.c_uint16), ("mer_len", C.c_uint8),
                ("status", C.c_uint8)]


class kc_lassm_stats(C.Structure):
    _fields_ = [("ends", C.c_uint64), ("status", C.c_uint64 * 6)] + [(n, C.c_uint64) for n in (
        "cands_overhang", "cands_mate", "cand_bases", "iterations", "ext_bases", "ctgs_extended")] + [("reserved", C.c_uint64 * 5)]


KC_LASSM_MAX_MER_LEN = 128
KC_LASSM_MAX_WALK = 4096
KC_LASSM_MAX_CANDS = 1 << 20
KC_LASSM_NO_CANDS, KC_LASSM_TOO_MANY, KC_LASSM_DEAD_END, KC_LASSM_FORK, KC_LASSM_LOOP, KC_LASSM_MAX_LEN = range(6)


class kc_link_params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("min_score", "min_len", "end_slack", "max_overlap", "max_splint_gap", "insert_avg", "max_insert")] + [
        ("max_read_alns", C.c_uint16), ("flags", C.c_uint16)]


class kc_ctg_link(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("from_", "to", "splints", "spans")] + [(n, C.c_int32) for n in (
        "splint_gap_min", "splint_gap_max", "span_gap_min", "span_gap_max")] + [("splint_gap_sum", C.c_int64), ("span_gap_sum", C.c_int64)]


class kc_link_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads", "reads_over_cap", "records", "none", "filtered", "passed", "splint_cands", "splints_gap_out",
                                          "span_cands", "spans_too_far", "links", "links_splint_only", "links_span_only", "links_both",
                                          "ends_linked", "reserved")]


KC_LINK_MAX_SLACK = 1024
KC_LINK_MAX_OVERLAP = 65535
KC_LINK_MAX_READ_ALNS = 64


class kc_scaf_params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("min_splints", "min_spans", "max_second_permille", "overlap_slack", "flags")] + [("reserved", C.c_uint32 * 3)]


class kc_scaffold_rec(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("first_member", "n_members", "len", "n_bases", "overlap_bases", "flags")] + [("reserved", C.c_uint32 * 2)]


class kc_scaf_member(C.Structure):
    _fields_ = [("ctg", C.c_uint32), ("join", C.c_int32), ("out_pos", C.c_uint32), ("orient", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class kc_scaf_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("contigs", "records", "qualifying", "ends_best", "ends_ambiguous", "ends_not_mutual", "edges_chosen",
                                          "overlaps_checked", "overlaps_rejected", "edges_joined", "scaffolds", "singletons", "circular",
                                          "bases", "n_bases", "overlap_bases", "longest")] + [("reserved", C.c_uint64 * 3)]


KC_SCAF_MAX_SLACK = 64
KC_SCAF_CIRCULAR = 1


class kc_close_params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("min_score", "min_len", "end_slack", "max_overlap", "max_splint_gap", "min_reads",
                                          "min_agree_permille")] + [("max_read_alns", C.c_uint16), ("flags", C.c_uint16)]


class kc_closure(C.Structure):
    _fields_ = [("cands", C.c_uint32), ("reads", C.c_uint32), ("old_join", C.c_int32), ("new_join", C.c_int32), ("fill_pos", C.c_uint32),
                ("disputed", C.c_uint32), ("status", C.c_uint8), ("pad", C.c_uint8 * 3), ("reserved", C.c_uint32)]


class kc_close_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("members", "joins", "gaps", "reads_over_cap", "passed", "cands", "cands_off_join", "gaps_no_reads",
                                          "gaps_weak", "filled", "abutted", "overlapped", "overlaps_rejected", "fill_bases", "n_bases_left",
                                          "disputed_cols")]


(KC_CLOSE_HEAD, KC_CLOSE_NOT_A_GAP, KC_CLOSE_NO_READS, KC_CLOSE_WEAK, KC_CLOSE_FILLED, KC_CLOSE_ABUT, KC_CLOSE_OVERLAP,
 KC_CLOSE_OVERLAP_REJECTED) = range(8)


class kc_shuffle_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("pairs", "homed", "homeless", "one_mate", "two_same", "two_diff", "homes", "max_home_pairs", "bytes",
                                          "key_bits")]


KC_SHUFFLE_MAX_PARTS = 65536
KC_SHUFFLE_NO_HOME = 0xFFFFFFFF


class kc_asm_params(C.Structure):
    _fields_ = [("min_len", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class kc_asm_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("contigs", "bases", "selected", "sel_bases", "a", "c", "g", "t", "n", "n_runs", "longest", "shortest",
                                          "n50", "l50", "n90", "l90")] + [("ge_count", C.c_uint64 * 5), ("ge_bases", C.c_uint64 * 5),
                                                                         ("key_bits", C.c_uint64), ("reserved", C.c_uint64 * 5)]


class kc_fasta_params(C.Structure):
    _fields_ = [("line_width", C.c_uint32), ("prefix_len", C.c_uint32), ("flags", C.c_uint32), ("reserved0", C.c_uint32), ("prefix", C.c_char * 32),
                ("reserved", C.c_uint32 * 4)]


KC_ASM_BY_LENGTH = 1
KC_ASM_CLASSES = (1000, 5000, 10000, 25000, 50000)
KC_FASTA_MAX_PREFIX = 32


class kc_fasta_in_params(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("default_depth", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class kc_fasta_in_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("lines", "empty_lines", "records", "empty_records", "bases", "lowered", "recoded", "longest", "with_id",
                                          "with_depth")] + [("reserved", C.c_uint64 * 6)]


class kc_fasta_rec(C.Structure):
    _fields_ = [("hdr_pos", C.c_uint64), ("hdr_len", C.c_uint32), ("seq_lines", C.c_uint32), ("id", C.c_uint64), ("depth", C.c_uint32),
                ("flags", C.c_uint32)]


KC_FASTA_PARTIAL = 1
KC_FASTA_STRICT = 2
KC_FASTA_HDR_SCAN = 256
KC_FASTA_HAS_ID = 1
KC_FASTA_HAS_DEPTH = 2
KC_FASTA_LOWERED = 4
KC_FASTA_RECODED = 8


class kc_fastq_out_params(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("prefix_len", C.c_uint32), ("first_id", C.c_uint64), ("prefix", C.c_char * 32), ("reserved", C.c_uint32 * 4)]


KC_FASTQ_OUT_PACKED = 1
KC_FASTQ_OUT_PAIRED = 2
KC_FASTQ_OUT_CHECK = 4
KC_FASTQ_OUT_MAX_PREFIX = 32


class kc_dedup_params(C.Structure):
    _fields_ = [("max_mismatches", C.c_uint32), ("flags", C.c_uint32), ("max_candidates", C.c_uint64), ("reserved", C.c_uint32 * 4)]


class kc_dedup_rec(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("status", "container", "pos", "mismatches", "new_index", "len", "absorbed")] + [
        ("orient", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class kc_dedup_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("contigs", "bases", "anchored", "unanchored", "windows", "window_hits", "candidates", "verified",
                                          "duplicates", "contained", "kept", "kept_bases", "removed_bases", "longest_removed")] + [
        ("reserved", C.c_uint64 * 2)]


KC_DEDUP_DUPLICATES_ONLY = 1
KC_DEDUP_KEPT, KC_DEDUP_DUPLICATE, KC_DEDUP_CONTAINED = range(3)
KC_DEDUP_UNANCHORED = 1
KC_DEDUP_NONE = 0xFFFFFFFF

class kc_kdepth_params(C.Structure):
    _fields_ = [("min_count", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class kc_kdepth_rec(C.Structure):
    _fields_ = [("sum", C.c_uint64), ("windows", C.c_uint32), ("present", C.c_uint32), ("solid", C.c_uint32), ("min_count", C.c_uint16),
                ("max_count", C.c_uint16), ("mean", C.c_uint16), ("reserved", C.c_uint16 * 3)]


class kc_kdepth_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("seqs", "bytes", "windows", "present", "solid", "sum", "longest", "reserved")]


class kc_spectrum_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("kmers", "sum_counts", "max_count", "mode_count", "mode_kmers", "saturated")] + [
        ("reserved", C.c_uint64 * 2)]


KC_KDEPTH_FILL_MEAN = 1
KC_SPECTRUM_BINS = 65536


class kc_correct_params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("min_count", "min_gain", "min_windows", "rounds", "max_qual", "flags")] + [("reserved", C.c_uint32 * 2)]


class kc_correct_rec(C.Structure):
    _fields_ = [("weak_before", C.c_uint32), ("weak_after", C.c_uint32), ("corrected", C.c_uint16), ("flags", C.c_uint16), ("reserved", C.c_uint32)]


class kc_correct_fix(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("pos", C.c_uint32), ("old_base", C.c_uint8), ("new_base", C.c_uint8), ("round", C.c_uint8), ("side", C.c_uint8),
                ("score", C.c_uint16), ("runner_up", C.c_uint16)]


class kc_correct_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("seqs", "bytes", "windows", "weak_before", "weak_after", "sites", "accepted", "rounds")]


(KC_CORRECT_UNANCHORED, KC_CORRECT_SHORT_RUN, KC_CORRECT_THIN, KC_CORRECT_QUAL_GATED, KC_CORRECT_NO_GAIN,
 KC_CORRECT_AMBIGUOUS) = (1 << i for i in range(6))
KC_CORRECT_MAX_ROUNDS = 8
KC_CORRECT_LEFT, KC_CORRECT_RIGHT = 0, 1



class kc_polish_params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("min_score", "min_len", "edge_clip", "max_mismatches", "min_depth", "min_permille", "min_qual", "flags")]


class kc_polish_ctg(C.Structure):
    _fields_ = [("votes", C.c_uint64)] + [(n, C.c_uint32) for n in ("placed", "changed", "filled", "disputed", "thin", "uncovered")]


class kc_polish_fix(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("ctg", C.c_uint32), ("old_base", C.c_uint8), ("new_base", C.c_uint8), ("top", C.c_uint16), ("tot", C.c_uint16),
                ("pad", C.c_uint16)]


class kc_polish_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("records", "none", "filtered", "not_best", "unequal", "divergent", "placed", "votes", "columns", "uncovered",
                                          "thin", "disputed", "confirmed", "changed", "filled", "sort_passes")]


KC_POLISH_BEST_ONLY = 1


class kc_break_params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("max_insert", "max_span", "min_disc", "margin", "min_run", "flags")] + [("reserved", C.c_uint32 * 2)]


class kc_break_piece(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("ctg", "start", "len", "flags")]


class kc_break_rec(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("ctg", "pos", "run_start", "run_len", "span", "disc", "piece", "pad")]


class kc_break_stats(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in ("pairs", "spanning", "discordant_pairs", "one_mate", "none", "disc_mates", "empty_intervals", "span_sum",
                                           "disc_sum")] +
                [(n, C.c_uint32) for n in ("columns", "interior", "weak", "runs", "short_runs", "breaks", "broken_contigs", "pieces")] +
                [("reserved", C.c_uint32 * 6)])


KC_BREAK_ONE_MATE = 1

# every symbol include/kcount_mi355.h declares: (restype, argtypes)
SYMBOLS = {
    "kc_abi_version": (C.c_int, []),
    "kc_error_string": (C.c_char_p, [C.c_int]),
    "kc_last_error": (C.c_char_p, []),
    "kc_debug_filled_bytes": (C.c_uint64, []),
    "kc_device_count": (C.c_int, []),
    "kc_num_longs": (C.c_int, [C.c_int]),
    "kc_record_longs": (C.c_int, [C.c_int]),
    "kc_owner": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "kc_owner_reference": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "kc_create": (C.c_void_p, [C.POINTER(kc_config), C.POINTER(C.c_int)]),
    "kc_destroy": (None, [C.c_void_p]),
    "kc_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kc_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "kc_submit_reads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "kc_submit_packed_reads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "kc_fastq_to_packed": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]),
    "kc_fastq_pairs": (C.c_int, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                  C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kc_fastq_to_packed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                             C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kc_fastq_pairs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kc_merge_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(kc_merge_stats)]),
    "kc_adapters_index": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64)]),
    "kc_adapters_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kc_adapters_clear": (C.c_int, [C.c_void_p]),
    "kc_trim_adapters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(kc_trim_stats)]),
    "kc_submit_seq_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "kc_extract_partition": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                       C.c_uint64, C.c_void_p]),
    "kc_extract_partition_seq_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]),
    "kc_insert_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "kc_shard_extract": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]),
    "kc_shard_extract_seq_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]),
    "kc_shard_reserve": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "kc_shard_commit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "kc_shard_owner": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "kc_wire_unit": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kc_partition_owner": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "kc_insert_record_pieces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "kc_shard_capacity": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "kc_build_supermers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32), C.c_void_p]),
    "kc_submit_packed_supermers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "kc_flush": (C.c_int, [C.c_void_p]),
    "kc_finalize": (C.c_int, [C.c_void_p, C.POINTER(kc_result)]),
    "kc_copy_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kc_begin_ctg_kmers": (C.c_int, [C.c_void_p, C.c_uint64]),
    "kc_submit_ctg_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "kc_ctg_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kc_arena_probe_rate": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "kc_copy_results_entries": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "kc_sort_results": (C.c_int, [C.c_void_p, C.POINTER(kc_result)]),
    "kc_dump_text_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "kc_build_unitigs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64), C.POINTER(kc_unitig_stats)]),
    "kc_ctg_index_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(kc_ctg_index_stats)]),
    "kc_ctg_index_clear": (C.c_int, [C.c_void_p]),
    "kc_align_reads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(kc_align_stats)]),
    "kc_align_gapped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32,
                                   C.POINTER(kc_aln_scores), C.c_uint32, C.c_void_p, C.POINTER(kc_gap_stats)]),
    "kc_ctg_index_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kc_aln_depths": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_void_p, C.c_void_p, C.POINTER(kc_depth_stats)]),
    "kc_pair_inserts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.POINTER(kc_insert_stats)]),
    "kc_local_assm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                 C.c_int, C.POINTER(kc_lassm_params), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                 C.POINTER(kc_lassm_stats)]),
    "kc_ctg_links": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.POINTER(kc_link_params), C.c_void_p,
                                C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(kc_link_stats)]),
    "kc_scaffold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(kc_scaf_params), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(kc_scaf_stats)]),
    "kc_close_gaps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int,
                                C.POINTER(kc_close_params), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_uint64), C.POINTER(kc_close_stats)]),
    "kc_shuffle_reads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(kc_shuffle_stats)]),
    "kc_ctg_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(kc_asm_params), C.c_void_p,
                                C.POINTER(C.c_uint64), C.POINTER(kc_asm_stats)]),
    "kc_fasta_text": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                C.POINTER(kc_fasta_params), C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kc_fasta_to_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(kc_fasta_in_params), C.c_void_p, C.c_uint64, C.c_void_p,
                                    C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.POINTER(kc_fasta_in_stats)]),
    "kc_fastq_text": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int,
                                C.POINTER(kc_fastq_out_params), C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kc_ctg_dedup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.POINTER(kc_dedup_params), C.c_void_p,
                               C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                               C.POINTER(kc_dedup_stats)]),
    "kc_seq_kmer_depths": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(kc_kdepth_params), C.c_void_p,
                                     C.c_void_p, C.POINTER(kc_kdepth_stats)]),
    "kc_count_spectrum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(kc_spectrum_stats)]),
    "kc_lookup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kc_dump_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "kc_get_stats": (C.c_int, [C.c_void_p, C.POINTER(kc_stats)]),
    "kc_set_tuning": (C.c_int, [C.c_void_p, C.POINTER(kc_tuning)]),
    "kc_get_kernel_times": (C.c_int, [C.c_void_p, C.POINTER(kc_kernel_time), C.c_int, C.POINTER(C.c_int)]),
    "kc_clear_kernel_times": (C.c_int, [C.c_void_p]),
    "kc_synth_default_params": (None, [C.POINTER(kc_synth_params)]),
    "kc_synth_reads_host": (C.c_int, [C.POINTER(kc_synth_params), C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kc_synth_reads_device": (C.c_int, [C.c_void_p, C.POINTER(kc_synth_params), C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
}

# every symbol include/kcount_mi355_correct.h declares, in the same form
SYMBOLS_CORRECT = {
    "kc_correct_reads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(kc_correct_params),
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(kc_correct_stats)]),
}

# every symbol include/kcount_mi355_polish.h declares, in the same form
SYMBOLS_POLISH = {
    "kc_ctg_polish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(kc_polish_params),
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(kc_polish_stats)]),
}

# every symbol include/kcount_mi355_break.h declares, in the same form
SYMBOLS_BREAK = {
    "kc_ctg_break": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(kc_break_params),
                               C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(kc_break_stats)]),
}


def lib_path():
    # KC_LIB: an alternative build of the same library (tuning experiments only)
    return os.environ.get("KC_LIB") or os.path.join(_HERE, "csrc", "libkcount_mi355.so")


def lib():
    """Load the HIP library.  Raises if it has not been built: there is no other implementation."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(or make -C mhm2_kmer_analysis_v2_amd/csrc); there is no CPU fallback" % p)
        L = C.CDLL(p)
        for name, (res, args) in list(SYMBOLS.items()) + list(SYMBOLS_CORRECT.items()) + list(SYMBOLS_POLISH.items()) + list(SYMBOLS_BREAK.items()):
            f = getattr(L, name)  # AttributeError if the .so does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def check(status, where):
    if status != KC_OK:
        raise KcError(status, where)
