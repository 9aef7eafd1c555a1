// kc_kinds.hpp -- the kinds under which the host times its kernel launches, and the name each is reported under.  One list:
// the enum and the names come from it, so a kind and its name cannot drift apart.  No HIP in here.
//
// Several kinds are one kernel launched by different callers or in different passes; the name in angle brackets says
// which (kc_align_lengths_kernel<close> is kc_close_gaps' launch of kc_align_lengths_kernel,
// <assembly> kc_ctg_select's, <fasta> kc_fasta_text's, <fasta in> kc_fasta_to_block's, <fastq out> kc_fastq_text's, <dedup> kc_ctg_dedup's, <correct> kc_correct_reads', <polish> kc_ctg_polish's, <break> kc_ctg_break's).  The *_scan_kernel names are
// the uses of the one shared kc_scan_kernel (kc_scan.hpp) and keep the names they were first reported under.
#pragma once

#define KC_KERNEL_KINDS(X) \
  X(KT_EXTRACT_INSERT,     "kc_extract_kernel<insert>") \
  X(KT_EXTRACT_BIN,        "kc_bin_reads_kernel") \
  X(KT_INSERT_RECORDS,     "kc_insert_records_kernel") \
  X(KT_FINALIZE,           "kc_finalize_kernel") \
  X(KT_TILE_FIRST,         "kc_tile_first_kernel") \
  X(KT_REHASH,             "kc_rehash_kernel") \
  X(KT_L1_READS,           "kc_l1_reads_kernel") \
  X(KT_L1_RECORDS,         "kc_l1_records_kernel") \
  X(KT_L2_SPLIT,           "kc_l2_split_kernel") \
  X(KT_COUNT_REGIONS,      "kc_count_kernel") \
  X(KT_FALLBACK,           "kc_flagged_to_table_kernel") \
  X(KT_SHARD_PACK,         "kc_shard_pack_kernel") \
  X(KT_L1_READS_UQ,        "kc_l1_reads_kernel<byte-loaded qualities>") \
  X(KT_L1_READS16,         "kc_l1_reads16_kernel") \
  X(KT_L2_REC6,            "kc_l2_rec6_kernel") \
  X(KT_BIN16,              "kc_bin16_kernel") \
  X(KT_L1_WIRE6,           "kc_l1_wire6_kernel") \
  X(KT_MERGE_DECIDE,       "kc_merge_decide_kernel") \
  X(KT_MERGE_DECIDE_LONG,  "kc_merge_decide_kernel<long>") \
  X(KT_MERGE_SCAN,         "kc_merge_scan_kernel") \
  X(KT_MERGE_WRITE,        "kc_merge_write_kernel") \
  X(KT_MERGE_WRITE_LONG,   "kc_merge_write_kernel<long>") \
  X(KT_FQ_COUNT,           "kc_fq_count_kernel") \
  X(KT_FQ_SCAN,            "kc_fq_scan_kernel") \
  X(KT_FQ_INDEX,           "kc_fq_index_kernel") \
  X(KT_FQ_CHECK,           "kc_fq_check_kernel") \
  X(KT_FQ_DETAIL,          "kc_fq_detail_kernel") \
  X(KT_FQ_SUMS,            "kc_fq_sums_kernel") \
  X(KT_FQ_WRITE_PACKED,    "kc_fq_write_kernel<packed>") \
  X(KT_FQ_WRITE_PAIRS,     "kc_fq_write_kernel<pairs>") \
  X(KT_TRIM_SEED,          "kc_trim_seed_kernel") \
  X(KT_TRIM_ALIGN,         "kc_trim_align_kernel") \
  X(KT_TRIM_SIZES,         "kc_trim_sizes_kernel") \
  X(KT_TRIM_SCAN,          "kc_merge_scan_kernel<trim>") \
  X(KT_TRIM_WRITE,         "kc_trim_write_kernel") \
  X(KT_SORT_HIST,          "kc_sort_hist_kernel") \
  X(KT_SORT_HIST_LOAD,     "kc_sort_hist_kernel<load>") \
  X(KT_SORT_SCAN,          "kc_sort_scan_kernel") \
  X(KT_SORT_SCATTER,       "kc_sort_scatter_kernel") \
  X(KT_SORT_GATHER,        "kc_sort_gather_kernel") \
  X(KT_DUMP_SIZES,         "kc_dump_sizes_kernel") \
  X(KT_DUMP_SCAN,          "kc_dump_scan_kernel") \
  X(KT_DUMP_WRITE,         "kc_dump_write_kernel") \
  X(KT_UNITIG_LINKS,       "kc_unitig_links_kernel") \
  X(KT_UNITIG_MIN_JUMP,    "kc_unitig_min_jump_kernel") \
  X(KT_UNITIG_CUT,         "kc_unitig_cut_kernel") \
  X(KT_UNITIG_RANK_JUMP,   "kc_unitig_rank_jump_kernel") \
  X(KT_UNITIG_SELECT,      "kc_unitig_select_kernel") \
  X(KT_UNITIG_SCAN,        "kc_unitig_scan_kernel") \
  X(KT_UNITIG_WRITE,       "kc_unitig_write_kernel") \
  X(KT_UNITIG_DEPTH,       "kc_unitig_depth_kernel") \
  X(KT_ALIGN_CHECK,        "kc_align_check_kernel") \
  X(KT_ALIGN_INDEX,        "kc_align_index_kernel") \
  X(KT_ALIGN_SWEEP,        "kc_align_sweep_kernel") \
  X(KT_ALIGN_LENGTHS,      "kc_align_lengths_kernel") \
  X(KT_ALIGN_COUNT,        "kc_align_reads_kernel<count>") \
  X(KT_ALIGN_SCAN,         "kc_align_scan_kernel") \
  X(KT_ALIGN_WRITE,        "kc_align_reads_kernel<write>") \
  X(KT_GAP_LENGTHS,        "kc_align_lengths_kernel<gap>") \
  X(KT_GAP_CHECK,          "kc_gap_check_kernel") \
  X(KT_GAP_SORT,           "kc_gap_sort_kernel") \
  X(KT_GAP_DP,             "kc_gap_dp_kernel") \
  X(KT_DEPTH_CHECK,        "kc_depth_check_kernel") \
  X(KT_DEPTH_BEST,         "kc_depth_best_kernel") \
  X(KT_DEPTH_MARK,         "kc_depth_mark_kernel") \
  X(KT_DEPTH_TILE_SUMS,    "kc_depth_tile_sums_kernel") \
  X(KT_DEPTH_SCAN,         "kc_depth_scan_kernel") \
  X(KT_DEPTH_RESCAN,       "kc_depth_rescan_kernel") \
  X(KT_DEPTH_CTG,          "kc_depth_ctg_kernel") \
  X(KT_DEPTH_FILL,         "kc_depth_fill_kernel") \
  X(KT_PAIR_LENGTHS,       "kc_align_lengths_kernel<pair>") \
  X(KT_PAIR_CHECK,         "kc_depth_check_kernel<pair>") \
  X(KT_PAIR_BEST,          "kc_depth_best_kernel<pair>") \
  X(KT_PAIR_CLASSIFY,      "kc_pair_classify_kernel") \
  X(KT_PAIR_CLASSIFY_LDS,  "kc_pair_classify_kernel<lds>") \
  X(KT_LASSM_LENGTHS,      "kc_align_lengths_kernel<lassm>") \
  X(KT_LASSM_CHECK,        "kc_depth_check_kernel<lassm>") \
  X(KT_LASSM_PAIR_CHECK,   "kc_lassm_pair_check_kernel") \
  X(KT_LASSM_COUNT,        "kc_lassm_cands_kernel<count>") \
  X(KT_LASSM_PLAN,         "kc_lassm_plan_kernel") \
  X(KT_LASSM_SCAN,         "kc_lassm_scan_kernel") \
  X(KT_LASSM_SCATTER,      "kc_lassm_cands_kernel<write>") \
  X(KT_LASSM_TEXT,         "kc_lassm_text_kernel") \
  X(KT_LASSM_WALK,         "kc_lassm_walk_kernel") \
  X(KT_LASSM_LENS,         "kc_lassm_lens_kernel") \
  X(KT_LASSM_ENDS,         "kc_lassm_ends_kernel") \
  X(KT_LASSM_WRITE,        "kc_lassm_write_kernel") \
  X(KT_LINK_LENGTHS,       "kc_align_lengths_kernel<links>") \
  X(KT_LINK_CHECK,         "kc_depth_check_kernel<links>") \
  X(KT_LINK_PAIR_CHECK,    "kc_lassm_pair_check_kernel<links>") \
  X(KT_LINK_GROUP_COUNT,   "kc_link_group_kernel<count>") \
  X(KT_LINK_GROUP_FILL,    "kc_link_group_kernel<fill>") \
  X(KT_LINK_TILE_SCAN,     "kc_link_tile_scan_kernel") \
  X(KT_LINK_SCAN,          "kc_link_scan_kernel") \
  X(KT_LINK_CANDS_COUNT,   "kc_link_cands_kernel<count>") \
  X(KT_LINK_CANDS_WRITE,   "kc_link_cands_kernel<write>") \
  X(KT_LINK_SORT_HIST,     "kc_sort_hist_kernel<links>") \
  X(KT_LINK_SORT_SCAN,     "kc_sort_scan_kernel<links>") \
  X(KT_LINK_SORT_SCATTER,  "kc_sort_scatter_kernel<links>") \
  X(KT_LINK_HEADS,         "kc_link_heads_kernel") \
  X(KT_LINK_REDUCE,        "kc_link_reduce_kernel") \
  X(KT_LINK_EMIT,          "kc_link_emit_kernel") \
  X(KT_LINK_END_FIRST,     "kc_link_end_first_kernel") \
  X(KT_SCAF_CHECK,         "kc_scaf_check_kernel") \
  X(KT_SCAF_END_FIRST,     "kc_link_end_first_kernel<scaffold>") \
  X(KT_SCAF_CHOOSE,        "kc_scaf_choose_kernel") \
  X(KT_SCAF_EDGE,          "kc_scaf_edge_kernel") \
  X(KT_SCAF_NEXT,          "kc_scaf_next_kernel") \
  X(KT_SCAF_MIN_JUMP,      "kc_unitig_min_jump_kernel<scaffold>") \
  X(KT_SCAF_CUT,           "kc_unitig_cut_kernel<scaffold>") \
  X(KT_SCAF_WEIGHT,        "kc_scaf_weight_kernel") \
  X(KT_SCAF_RANK_JUMP,     "kc_unitig_rank_jump_kernel<scaffold>") \
  X(KT_SCAF_POS_JUMP,      "kc_unitig_rank_jump_kernel<scaffold pos>") \
  X(KT_SCAF_SELECT,        "kc_scaf_select_kernel") \
  X(KT_SCAF_SCAN,          "kc_scaf_scan_kernel") \
  X(KT_SCAF_MEMBERS,       "kc_scaf_members_kernel") \
  X(KT_SCAF_RECORDS,       "kc_scaf_records_kernel") \
  X(KT_SCAF_WRITE,         "kc_scaf_write_kernel") \
  X(KT_CLOSE_LENGTHS,      "kc_align_lengths_kernel<close>") \
  X(KT_CLOSE_CHECK,        "kc_depth_check_kernel<close>") \
  X(KT_CLOSE_CHECK_SCAF,   "kc_close_check_scaf_kernel") \
  X(KT_CLOSE_CLAIM,        "kc_close_claim_kernel") \
  X(KT_CLOSE_CHECK_MEMBER, "kc_close_check_member_kernel") \
  X(KT_CLOSE_GROUP_COUNT,  "kc_link_group_kernel<close count>") \
  X(KT_CLOSE_GROUP_FILL,   "kc_link_group_kernel<close fill>") \
  X(KT_CLOSE_TILE_SCAN,    "kc_link_tile_scan_kernel<close>") \
  X(KT_CLOSE_SCAN,         "kc_close_scan_kernel") \
  X(KT_CLOSE_ENDS,         "kc_close_ends_kernel") \
  X(KT_CLOSE_CANDS_COUNT,  "kc_close_cands_kernel<count>") \
  X(KT_CLOSE_CANDS_WRITE,  "kc_close_cands_kernel<write>") \
  X(KT_CLOSE_DECIDE,       "kc_close_decide_kernel") \
  X(KT_CLOSE_PLACE,        "kc_close_place_kernel") \
  X(KT_CLOSE_VOTE,         "kc_close_vote_kernel") \
  X(KT_CLOSE_RECORDS,      "kc_close_records_kernel") \
  X(KT_CLOSE_WRITE,        "kc_close_write_kernel") \
  X(KT_SHUF_LENGTHS,       "kc_align_lengths_kernel<shuffle>") \
  X(KT_SHUF_CHECK,         "kc_depth_check_kernel<shuffle>") \
  X(KT_SHUF_PAIR_CHECK,    "kc_lassm_pair_check_kernel<shuffle>") \
  X(KT_SHUF_LONGEST,       "kc_shuf_longest_kernel") \
  X(KT_SHUF_KEY,           "kc_shuf_key_kernel") \
  X(KT_SHUF_SORT_HIST,     "kc_sort_hist_kernel<shuffle>") \
  X(KT_SHUF_SORT_SCAN,     "kc_sort_scan_kernel<shuffle>") \
  X(KT_SHUF_SORT_SCATTER,  "kc_sort_scatter_kernel<shuffle>") \
  X(KT_SHUF_PLACE,         "kc_shuf_place_kernel") \
  X(KT_SHUF_TILE_SCAN,     "kc_link_tile_scan_kernel<shuffle>") \
  X(KT_SHUF_SCAN,          "kc_shuf_scan_kernel") \
  X(KT_SHUF_OFFSETS,       "kc_shuf_offsets_kernel") \
  X(KT_SHUF_GATHER,        "kc_shuf_gather_kernel") \
  X(KT_SHUF_REMAP,         "kc_shuf_remap_kernel") \
  X(KT_SHUF_PARTS,         "kc_shuf_parts_kernel") \
  X(KT_ASM_CHECK,          "kc_align_check_kernel<assembly>") \
  X(KT_ASM_LENS,           "kc_asm_lens_kernel") \
  X(KT_ASM_TILE_SCAN,      "kc_link_tile_scan_kernel<assembly>") \
  X(KT_ASM_SCAN,           "kc_asm_scan_kernel") \
  X(KT_ASM_COMPACT,        "kc_asm_compact_kernel") \
  X(KT_ASM_SORT_HIST,      "kc_sort_hist_kernel<assembly>") \
  X(KT_ASM_SORT_SCAN,      "kc_sort_scan_kernel<assembly>") \
  X(KT_ASM_SORT_SCATTER,   "kc_sort_scatter_kernel<assembly>") \
  X(KT_ASM_SORTED,         "kc_asm_sorted_kernel") \
  X(KT_ASM_LEN_TILE_SCAN,  "kc_link_tile_scan_kernel<assembly lengths>") \
  X(KT_ASM_LEN_SCAN,       "kc_asm_scan_kernel<lengths>") \
  X(KT_ASM_NX,             "kc_asm_nx_kernel") \
  X(KT_ASM_SPANS,          "kc_asm_spans_kernel") \
  X(KT_ASM_COMP,           "kc_asm_comp_kernel") \
  X(KT_ASM_TEXT_CHECK,     "kc_asm_text_check_kernel") \
  X(KT_ASM_SIZES,          "kc_asm_sizes_kernel") \
  X(KT_ASM_TEXT_TILE_SCAN, "kc_link_tile_scan_kernel<fasta>") \
  X(KT_ASM_TEXT_SCAN,      "kc_asm_scan_kernel<fasta>") \
  X(KT_ASM_STARTS,         "kc_asm_starts_kernel") \
  X(KT_ASM_TEXT_SPANS,     "kc_asm_spans_kernel<fasta>") \
  X(KT_ASM_WRITE,          "kc_asm_write_kernel") \
  X(KT_FA_COUNT,           "kc_fq_count_kernel<fasta in>") \
  X(KT_FA_SCAN,            "kc_fq_scan_kernel<fasta in>") \
  X(KT_FA_INDEX,           "kc_fq_index_kernel<fasta in>") \
  X(KT_FA_LINES,           "kc_fa_lines_kernel") \
  X(KT_FA_TILE_SCAN,       "kc_link_tile_scan_kernel<fasta in>") \
  X(KT_FA_LINE_SCAN,       "kc_fa_scan_kernel") \
  X(KT_FA_STARTS,          "kc_fa_starts_kernel") \
  X(KT_FA_SPANS,           "kc_fa_spans_kernel") \
  X(KT_FA_CHECK,           "kc_fa_check_kernel") \
  X(KT_FA_DETAIL,          "kc_fa_detail_kernel") \
  X(KT_FA_RECS,            "kc_fa_recs_kernel") \
  X(KT_FA_BLOCK_SPANS,     "kc_fa_spans_kernel<block>") \
  X(KT_FA_WRITE,           "kc_fa_write_kernel") \
  X(KT_RTEXT_CHECK,        "kc_rtext_check_kernel") \
  X(KT_RTEXT_BYTES,        "kc_rtext_bytes_kernel") \
  X(KT_RTEXT_DETAIL,       "kc_rtext_detail_kernel") \
  X(KT_RTEXT_SIZES,        "kc_rtext_sizes_kernel") \
  X(KT_RTEXT_TILE_SCAN,    "kc_link_tile_scan_kernel<fastq out>") \
  X(KT_RTEXT_SCAN,         "kc_asm_scan_kernel<fastq out>") \
  X(KT_RTEXT_STARTS,       "kc_rtext_starts_kernel") \
  X(KT_RTEXT_SPANS,        "kc_asm_spans_kernel<fastq out>") \
  X(KT_RTEXT_WRITE,        "kc_rtext_write_kernel") \
  X(KT_DEDUP_CHECK,        "kc_align_check_kernel<dedup>") \
  X(KT_DEDUP_ANCHOR,       "kc_dedup_anchor_kernel") \
  X(KT_DEDUP_LINK,         "kc_dedup_link_kernel") \
  X(KT_DEDUP_COUNT,        "kc_dedup_windows_kernel<count>") \
  X(KT_DEDUP_WRITE,        "kc_dedup_windows_kernel<write>") \
  X(KT_DEDUP_VERIFY,       "kc_dedup_verify_kernel") \
  X(KT_DEDUP_VERIFY_LONG,  "kc_dedup_verify_kernel<long>") \
  X(KT_DEDUP_BEST,         "kc_dedup_best_kernel") \
  X(KT_DEDUP_PICK,         "kc_dedup_pick_kernel") \
  X(KT_DEDUP_STATUS,       "kc_dedup_status_kernel") \
  X(KT_DEDUP_TILE_SCAN,    "kc_link_tile_scan_kernel<dedup>") \
  X(KT_DEDUP_SCAN,         "kc_dedup_scan_kernel") \
  X(KT_DEDUP_RECORDS,      "kc_dedup_records_kernel") \
  X(KT_DEDUP_GATHER,       "kc_dedup_gather_kernel") \
  X(KT_DEDUP_GATHER_DEPTHS, "kc_dedup_gather_kernel<depths>") \
  X(KT_KTRACK_OFFSETS,     "kc_ktrack_offsets_kernel") \
  X(KT_KTRACK_WINDOWS,     "kc_ktrack_windows_kernel") \
  X(KT_KTRACK_WINDOWS_FILL, "kc_ktrack_windows_kernel<fill>") \
  X(KT_KTRACK_RECORDS,     "kc_ktrack_records_kernel") \
  X(KT_KTRACK_FILL,        "kc_ktrack_fill_kernel") \
  X(KT_SPECT_HIST,         "kc_spect_hist_kernel") \
  X(KT_SPECT_STATS,        "kc_spect_stats_kernel") \
  X(KT_CORRECT_OFFSETS,    "kc_ktrack_offsets_kernel<correct>") \
  X(KT_CORRECT_TRACK,      "kc_ktrack_windows_kernel<correct>") \
  X(KT_CORRECT_SITES_COUNT, "kc_correct_sites_kernel<count>") \
  X(KT_CORRECT_SITES_SCAN, "kc_correct_scan_kernel<sites>") \
  X(KT_CORRECT_SITES_WRITE, "kc_correct_sites_kernel<write>") \
  X(KT_CORRECT_EVAL,       "kc_correct_eval_kernel") \
  X(KT_CORRECT_ACCEPT_SCAN, "kc_correct_scan_kernel<accepted>") \
  X(KT_CORRECT_APPLY,      "kc_correct_apply_kernel") \
  X(KT_CORRECT_RECORDS,    "kc_correct_records_kernel") \
  X(KT_POLISH_LENGTHS,     "kc_align_lengths_kernel<polish>") \
  X(KT_POLISH_CHECK,       "kc_depth_check_kernel<polish>") \
  X(KT_POLISH_BEST,        "kc_depth_best_kernel<polish>") \
  X(KT_POLISH_PLACE,       "kc_polish_place_kernel") \
  X(KT_POLISH_SORT_HIST,   "kc_sort_hist_kernel<polish>") \
  X(KT_POLISH_SORT_SCAN,   "kc_sort_scan_kernel<polish>") \
  X(KT_POLISH_SORT_SCATTER, "kc_sort_scatter_kernel<polish>") \
  X(KT_POLISH_TILE_COUNT,  "kc_polish_tile_kernel<count>") \
  X(KT_POLISH_TILE_SCAN,   "kc_link_tile_scan_kernel<polish>") \
  X(KT_POLISH_SCAN,        "kc_polish_scan_kernel") \
  X(KT_POLISH_TILE_WRITE,  "kc_polish_tile_kernel<write>") \
  X(KT_BREAK_LENGTHS,      "kc_align_lengths_kernel<break>") \
  X(KT_BREAK_CHECK,        "kc_depth_check_kernel<break>") \
  X(KT_BREAK_PAIR_CHECK,   "kc_lassm_pair_check_kernel<break>") \
  X(KT_BREAK_MARK,         "kc_break_mark_kernel") \
  X(KT_BREAK_TILE_SUMS,    "kc_break_tile_sums_kernel") \
  X(KT_BREAK_SCAN,         "kc_break_scan_kernel") \
  X(KT_BREAK_RESCAN,       "kc_break_rescan_kernel") \
  X(KT_BREAK_TILE_MAX,     "kc_break_tile_max_kernel") \
  X(KT_BREAK_RUNS_COUNT,   "kc_break_runs_kernel<count>") \
  X(KT_BREAK_RUNS_SCAN,    "kc_break_scan_kernel<runs>") \
  X(KT_BREAK_RUNS_WRITE,   "kc_break_runs_kernel<write>") \
  X(KT_BREAK_RECORDS,      "kc_break_records_kernel") \
  X(KT_BREAK_GATHER,       "kc_break_gather_kernel") \
  X(KT_BREAK_GATHER_DEPTHS, "kc_break_gather_kernel<depths>") \
  X(KT_BREAK_TRACKS,       "kc_break_tracks_kernel")

enum {
#define X(kind, name) kind,
  KC_KERNEL_KINDS(X)
#undef X
  KT_COUNT
};

static const char *const kt_names[] = {
#define X(kind, name) name,
    KC_KERNEL_KINDS(X)
#undef X
};
static_assert(sizeof(kt_names) / sizeof(kt_names[0]) == KT_COUNT, "a name for every kind");
