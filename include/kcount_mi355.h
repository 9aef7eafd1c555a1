/*
 * kcount_mi355.h -- C ABI of libkcount_mi355.so, the MI355X (gfx950) k-mer
 * analysis stage that drops in behind MHM2's kcount / KmerDHT operator surface.
 *
 * Plain C: opaque handle, plain pointers and sizes, int status codes, no
 * exceptions, no STL, no torch types.  Every entry point names the reference
 * interface it replaces (paths relative to the reference checkout).  The C++
 * adapters that re-create the reference's own driver classes on top of this
 * ABI are in mhm2_kmer_analysis_v2_amd/csrc/kcount_driver.hpp; the binding a
 * reference maintainer would add is shown in INTEGRATION.md.
 *
 * Semantics are those of the reference *CPU* backend (src/kcount/kcount_cpu.cpp),
 * spec S1-S9 in SURVEY.md section 8a -- not the reference GPU backend, which
 * differs from it (N handling, counter saturation).
 */
#ifndef KCOUNT_MI355_H
#define KCOUNT_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KC_ABI_VERSION 1

/* status codes (all entry points returning int) */
enum {
  KC_OK = 0,
  KC_ERR_INVALID_ARG = -1,
  KC_ERR_UNSUPPORTED_K = -2, /* k < 3 or k > 125 (126 and 127 would need a fifth record word) */
  KC_ERR_NO_DEVICE = -3,     /* HIP runtime reports no usable gfx950 device */
  KC_ERR_HIP = -4,           /* a HIP call failed; kc_last_error() has the text */
  KC_ERR_OUT_OF_MEMORY = -5,
  KC_ERR_CAPACITY = -6,      /* a buffer is too small: a caller-provided segment (retry with more room), or the k-mer buffer /
                                its overflow lists (raise max_kmers_buffered); kc_last_error says which */
  KC_ERR_BAD_BASE = -7,      /* a read holds a byte outside ACGTN/acgtn (reference: DIE at kcount_cpu.cpp:484-486) */
  KC_ERR_STATE = -8          /* call not allowed in this state (e.g. submit after finalize without reset) */
};

typedef struct kc_ctx kc_ctx;

/*
 * Run-time configuration.  Replaces the compile-time / CLI knobs the reference
 * spreads over CMakeDefinitions.txt and src/options.cpp:
 *   kmer_len     Options::kmer_lens                       src/options.hpp:80
 *   qual_offset  Options::qual_offset, SeqBlockInserter   src/kcount/kcount.hpp:60
 *   dmin_thres   --min-depth-thres, _dmin_thres           src/kcount/kmer_dht.hpp:57, src/kcount/kcount.cpp:146
 *   rank_me/n    upcxx::rank_me()/rank_n() as passed to
 *                HashTableGPUDriver::init                 src/kcount/kcount-gpu/gpu_hash_table.hpp:155
 *   max_elems    init(max_elems, ..., num_errors, ...)    same; here: expected distinct k-mers of this shard
 *                (0 = pick a default; the table grows instead of dropping inserts)
 */
typedef struct kc_config {
  int32_t kmer_len;
  int32_t qual_offset; /* 33 or 64 */
  int32_t dmin_thres;  /* default 2 */
  int32_t device;      /* HIP device ordinal */
  int32_t rank_me;     /* this shard owns k-mers with kc_owner(key) == rank_me */
  int32_t rank_n;      /* shards in the job (GPUs); 1 = everything local */
  uint64_t max_elems;
  uint32_t flags; /* KC_FLAG_* */
  uint32_t reserved;
  /* k-mer occurrences the context buffers on its fast (bucketed) path.  Sized for the whole input of a pass
   * (kc_reset .. kc_finalize) the stage runs in one pass, which is what the benchmark measures.  When more arrives,
   * what is buffered is counted, merged into the global table (one table operation per distinct k-mer) and the
   * buffer starts again empty: the reference streams 1 MB insert blocks into its one table for as long as reads come
   * (gpu_hash_table.cpp:681-695).  Correct for any size, but several times slower than one pass (the table then holds
   * every distinct k-mer, singletons included).  Role of the reference's my_num_kmers estimate
   * (src/contigging.cpp:86).  0 = 64 Mi. */
  uint64_t max_kmers_buffered;
} kc_config;

#define KC_FLAG_NONE 0u
#define KC_FLAG_REFERENCE_OWNER 2u /* owner shard = the reference's KmerDHT::get_kmer_target_rank (quick_hash of the minimizer,
                                     src/kcount/kmer_dht.cpp:117-119,192-196) instead of the k-mer hash: for runs mixed with
                                     unmodified MHM2 ranks; slower (k-m+1 m-mer comparisons per k-mer) */
#define KC_FLAG_SHARD_BUCKETS 4u /* this context will run the single-pass shard flow (kc_shard_*): its regions are sized for 1/rank_n
                                 * of the level-1 buckets holding all of max_elems (see kc_shard_capacity) */
#define KC_FLAG_WIRE_UNITS 8u /* kc_extract_partition / kc_insert_records exchange UNITS of the library's own wire record where the
                                 geometry has one (kc_wire_unit: four six-byte records of a mixed k-mer per three words for k = 21;
                                 one k-mer record otherwise) and the owner of a k-mer is kc_partition_owner, not kc_owner -- for the reads'
                                 k-mers that kc_extract_partition sends and for the contig k-mers that kc_submit_ctg_block keeps.
                                 All shards of an exchange must be created alike. */
#define KC_FLAG_TIME_KERNELS 1u /* bracket every kernel launch with HIP events on its own stream (kc_get_kernel_times) */

/* Scalars the reference logs (src/kcount/kcount.cpp:94-102,158-160;
 * src/kcount/kcount_cpu.cpp:495-521,586-598) plus table geometry. */
typedef struct kc_stats {
  uint64_t num_reads;
  uint64_t num_bases;
  uint64_t raw_kmers;      /* sum over reads of max(0, len-k+1): kcount.cpp:86 -- the unit of the k-mers/s metric */
  uint64_t kmers_inserted; /* k-mer occurrences with both neighbours (S5) put into this shard's table */
  uint64_t num_unique;     /* table entries before the purge */
  uint64_t num_purged;     /* entries removed by S8 */
  uint64_t total_kmers;    /* results: "Total kmers" */
  uint64_t sum_counts;     /* "Total kmer count sum" */
  uint64_t num_dropped;    /* always 0: the table grows; kept for the reference's precondition check */
  uint64_t capacity;       /* table slots */
  uint64_t num_gpu_calls;  /* kernel launches so far (HashTableGPUDriver::get_num_gpu_calls) */
  uint64_t table_bytes;
} kc_stats;

/* Dense result arrays resident in HBM (replaces the compact KmerExtsMap the
 * reference copies back slot by slot, gpu_hash_table.cpp:205-245,776-827, and
 * the KmerCounts it becomes, kmer_dht.hpp:62-68).  Unordered, like a hash-map
 * iteration; entry i is keys[i*num_longs .. +num_longs), counts[i], left[i],
 * right[i] with left/right in "ACGT".  Pointers stay valid until kc_reset /
 * kc_destroy, or a successful kc_sort_results (which orders them by key). */
typedef struct kc_result {
  uint64_t n;
  int32_t num_longs;
  int32_t reserved;
  const uint64_t *d_keys;
  const uint16_t *d_counts;
  const uint8_t *d_left;
  const uint8_t *d_right;
} kc_result;

/* ---- library ------------------------------------------------------------ */
int kc_abi_version(void);
const char *kc_error_string(int status);
const char *kc_last_error(void); /* text of the last failing HIP call on this thread */
int kc_device_count(void);       /* 0 without a GPU; never aborts */
/* KC_DEBUG_FILL=<byte> in the environment (decimal or 0x.., 0..255; read at every allocation): every device or pinned
 * allocation the library makes is filled with that byte before anything uses it, so that a result which depends on memory
 * the library has not written differs from its expectation instead of passing on what the allocator handed out (DESIGN.md,
 * "Poisoned scratch").  A block the library keeps is not filled again.  Unset or unparsable: nothing is filled.  This is
 * the number of bytes filled since the library was loaded: 0 without the variable; a test that sets it checks that the
 * figure rose, and so that its calls allocated at all. */
uint64_t kc_debug_filled_bytes(void);

/* Kmer<MAX_K>::N_LONGS for the MAX_K the reference would pick: k/32+1 (src/main.cpp:169-190, src/kmer.hpp:64). */
int kc_num_longs(int kmer_len);
/* Words of one k-mer RECORD on the shard wire (kc_extract_partition / kc_insert_records): kc_num_longs, plus one when
 * k % 32 is 30 or 31 (the last key word then has no six spare bits for the two extension codes, which ride in a word of
 * their own).  Results, dumps and lookups always use kc_num_longs. */
int kc_record_longs(int kmer_len);
/* Shard that owns a canonical k-mer (role of KmerDHT::get_kmer_target_rank,
 * src/kcount/kmer_dht.cpp:192-196; any deterministic function of the k-mer
 * gives the same final set).  Host-callable. */
int kc_owner(const uint64_t *kmer_words, int kmer_len, int rank_n);
/* The reference's own target rank, bit for bit: quick_hash(minimizer(kmer, m)) % rank_n with m = clamp(2k/3+1, 15, 27)
 * (src/kmer.cpp:349-398,459-468, src/hash_funcs.c:332-342, src/kcount/kmer_dht.cpp:117-119,192-196).  Host-callable;
 * contexts created with KC_FLAG_REFERENCE_OWNER use it on the device. */
int kc_owner_reference(const uint64_t *kmer_words, int kmer_len, int rank_n);

/* ---- context ------------------------------------------------------------ */
/* HashTableGPUDriver::init + ParseAndPackGPUDriver ctor (gpu_hash_table.cpp:522-624, parse_and_pack.cpp:239-267). */
kc_ctx *kc_create(const kc_config *cfg, int *status);
/* ~HashTableGPUDriver / ~ParseAndPackGPUDriver */
void kc_destroy(kc_ctx *ctx);
/* Launch everything on this hipStream_t (e.g. torch's current stream).  NULL = the context's own stream. */
int kc_set_stream(kc_ctx *ctx, void *hip_stream);
/* Empty the table and results but keep every allocation (multi-k sweeps with a new
 * kmer_len re-use the arena; the reference re-allocates per run, F5 in SURVEY.md). */
int kc_reset(kc_ctx *ctx, int new_kmer_len);

/* ---- the hot path ------------------------------------------------------- */
/*
 * count_kmers' read loop + SeqBlockInserter::process_seq + the whole insert path
 * for reads whose k-mers this shard owns (src/kcount/kcount.cpp:71-90,
 * kcount_cpu.cpp:73-103,338-355).  bases/quals: concatenated ASCII, read r is
 * [offsets[r], offsets[r+1]); quality mask S2 is applied on the device.
 * on_device != 0: all three pointers are device pointers (HBM-resident input).
 * With rank_n > 1 only k-mers owned by rank_me are inserted (use
 * kc_extract_partition + kc_insert_records for the sharded flow).
 */
int kc_submit_reads(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads,
                    int on_device);

/*
 * The same from the reference's in-memory read cache, fed to the device as it is stored: one byte per base,
 * low 3 bits = A0 C1 G2 T3 N4, high 5 bits = min(quality - qual_offset, 31) (PackedRead,
 * src/packed_reads.cpp:99-126), read r = packed[offsets[r], offsets[r+1]).  Saves count_kmers the per-read
 * unpack into three strings (src/kcount/kcount.cpp:76-85, packed_reads.cpp:196-208) and half the input bytes.
 */
int kc_submit_packed_reads(kc_ctx *ctx, const uint8_t *packed, const uint64_t *offsets, uint64_t nreads, int on_device);

/*
 * FASTQ text -> the read cache's packed bytes, on the host (no context, no GPU): the unpaired pass of
 * FastqReader::get_next_fq_record (src/fastq.cpp:1028-1140: four lines per record, '@' name, sequence, '+' line,
 * qualities of the sequence's length; trailing white space and CR stripped) followed by PackedRead's constructor
 * (src/packed_reads.cpp:99-126: ACGT 0-3, N and the IUPAC codes 4, quality min(q - qual_offset, 31) << 3).  The reads
 * are appended to packed[0..packed_capacity) with offsets[r] .. offsets[r+1] (offsets[0] = 0, reads_capacity + 1 entries),
 * ready for kc_submit_packed_reads.  *nreads / *nbytes receive the totals of the whole text even when the arrays are too
 * small (KC_ERR_CAPACITY: call again with that much room; call with NULL arrays to size).  KC_ERR_BAD_BASE: a character
 * the reference DIEs on; KC_ERR_INVALID_ARG: a malformed record (kc_last_error names the line).
 * The reference's dummy mate of an unpaired read (the one-base read "N", src/merge_reads.cpp:372-377) holds no k-mer
 * and is not produced.
 */
int kc_fastq_to_packed(const char *text, uint64_t len, int qual_offset, uint8_t *packed, uint64_t packed_capacity, uint64_t *offsets,
                       uint64_t reads_capacity, uint64_t *nreads, uint64_t *nbytes);

/*
 * Paired FASTQ text -> interleaved ASCII reads, on the host (no context, no GPU): the input of kc_merge_pairs.
 * text2 == NULL: text1 holds the pairs interleaved (mate 1, mate 2, mate 1, ...); else text1 holds the mates 1 and
 * text2 the mates 2, record by record.  bases / quals (capacity bytes each) receive the sequences and the quality
 * bytes as they are, offsets (reads_capacity + 1 entries) the read boundaries; read 2p is mate 1 of pair p and read
 * 2p+1 its mate 2.  Validation and the size query are those of kc_fastq_to_packed (NULL arrays: only *nreads /
 * *nbytes; KC_ERR_CAPACITY: call again with that much room).  Two files with different record counts, or an
 * interleaved file with an odd count, are KC_ERR_INVALID_ARG.  Record names are not checked (the reference's name
 * repair, src/merge_reads.cpp:386-467, is not part of this stage).
 */
int kc_fastq_pairs(const char *text1, uint64_t len1, const char *text2, uint64_t len2, uint8_t *bases, uint8_t *quals,
                   uint64_t capacity, uint64_t *offsets, uint64_t reads_capacity, uint64_t *nreads, uint64_t *nbytes);

#define KC_FASTQ_PARTIAL 1u /* the text is a prefix of a longer input: parse only its whole records */

/*
 * FASTQ text -> the read cache's packed bytes, parsed on the device: the reference's FastqReader::get_next_fq_record
 * (src/fastq.cpp:1028-1140) and PackedRead (src/packed_reads.cpp:99-126), in parallel over the text
 * (csrc/kc_fastq.hpp).  The device twin of kc_fastq_to_packed with the context's qual_offset: for every input, well
 * formed or not, the same status, *nreads, *nbytes, output bytes, offsets and kc_last_error() text.  NULL arrays are
 * a size query; KC_ERR_CAPACITY fills in the totals; a format error wins over KC_ERR_CAPACITY.
 * text: device memory read in place (on_device = 1), or host memory copied to the device first.  Any length, 2^32
 * bytes and more.  Output is device memory: d_packed (packed_capacity bytes) and d_offsets (reads_capacity + 1 entries,
 * d_offsets[0] = 0).
 * flags KC_FASTQ_PARTIAL: only whole records count, those whose four lines all end in '\n' inside the text; an
 * unfinished tail is neither parsed nor an error.  *consumed receives the byte just past the last whole record, and
 * the call equals the flag-free call on text[0, *consumed): a caller streams a file by carrying the tail into the
 * next call and making the last call without the flag.  Without the flag *consumed = len.  consumed may be NULL.
 * The context's table and state are not touched, so this may be called in any state.  The call runs on the context's
 * stream (kc_set_stream) and returns when its work there is done; device text written on another stream must be
 * complete before the call.
 */
int kc_fastq_to_packed_device(kc_ctx *ctx, const char *text, uint64_t len, int on_device, uint32_t flags, uint8_t *d_packed,
                              uint64_t packed_capacity, uint64_t *d_offsets, uint64_t reads_capacity, uint64_t *nreads,
                              uint64_t *nbytes, uint64_t *consumed);

/*
 * Paired FASTQ text -> interleaved ASCII reads, parsed on the device: FastqReader::get_next_fq_record
 * (src/fastq.cpp:1028-1140) for the input of kc_merge_pairs.  The device twin of kc_fastq_pairs (text2 == NULL:
 * text1 holds the pairs interleaved), identical to it as kc_fastq_to_packed_device is to kc_fastq_to_packed.
 * Input residence, output memory and the context as for kc_fastq_to_packed_device.  KC_FASTQ_PARTIAL: an interleaved
 * file is consumed up to its last whole pair; two files are each consumed up to the same record count, the smaller of
 * their whole-record counts (*consumed1, *consumed2).
 */
int kc_fastq_pairs_device(kc_ctx *ctx, const char *text1, uint64_t len1, const char *text2, uint64_t len2, int on_device,
                          uint32_t flags, uint8_t *d_bases, uint8_t *d_quals, uint64_t capacity, uint64_t *d_offsets,
                          uint64_t reads_capacity, uint64_t *nreads, uint64_t *nbytes, uint64_t *consumed1, uint64_t *consumed2);

/* Counters of kc_merge_pairs, the reference's merge_reads counters (src/merge_reads.cpp:469-648) */
typedef struct kc_merge_stats {
  uint64_t pairs;       /* pairs submitted */
  uint64_t merged;      /* num_merged */
  uint64_t ambiguous;   /* num_ambiguous: every increment the reference makes */
  uint64_t dropped;     /* both mates shorter than min_kmer_len (:473) */
  uint64_t overlap_len; /* sum of the merged pairs' overlaps */
  uint64_t merged_len;  /* sum of the merged reads' lengths */
  uint64_t out_reads;   /* reads written: 2 * pairs - merged - 2 * dropped */
  uint64_t out_bases;
} kc_merge_stats;

/*
 * Overlap merge of read pairs on the device: the pair loop of merge_reads (src/merge_reads.cpp:469-648) with no
 * adapter file (Adapters::trim_pair, the step in front of it, is kc_trim_adapters), writing the read cache's packed bytes (code | min(q - qual_offset, 31) << 3, as kc_fastq_to_packed)
 * ready for kc_submit_packed_reads(..., on_device = 1).  The exact rules are in csrc/kc_merge.hpp's header comment.
 * Input: interleaved mates (kc_fastq_pairs' layout, the one kc_submit_reads takes): 2 * npairs reads, ASCII bases
 * and qualities, offsets of 2 * npairs + 1 entries; device memory (on_device = 1) or host memory, which is staged.
 * min_kmer_len: a pair whose mates are both shorter is dropped (0 = the context's k).  The context's qual_offset is
 * used; nothing else of the context changes.
 * Output, always device memory, in pair order: one read for a merged pair, both mates as they came (mate 2 not
 * reverse-complemented) for an unmerged pair, nothing for a dropped pair; d_out_offsets gets *nreads + 1 entries.
 * The reference's one-base dummy mate after a merged pair holds no k-mer and is not produced.  Output bytes never
 * exceed the input's bases and output reads never exceed 2 * npairs.
 * KC_ERR_CAPACITY: the arrays are too small (or NULL); *nreads, *nbytes and *stats hold the totals.
 * KC_ERR_BAD_BASE: a byte outside kc_fastq_to_packed's table.  KC_ERR_INVALID_ARG: a quality outside
 * [qual_offset, qual_offset + 80] or a mate longer than 32767 -- stricter than the reference, which asserts or DIEs
 * only where its loop meets one.
 */
int kc_merge_pairs(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t npairs, int on_device,
                   int min_kmer_len, uint8_t *d_packed, uint64_t packed_capacity, uint64_t *d_out_offsets, uint64_t reads_capacity,
                   uint64_t *nreads, uint64_t *nbytes, kc_merge_stats *stats);

/*
 * Adapter FASTA text -> the adapter index, on the host (no context, no GPU): the first half of kc_adapters_load, on
 * its own so that the loading rules can be checked without a device.  Replaces Adapters::load_adapter_seqs
 * (src/adapters.cpp:48-146): lines as getline yields them, '>' lines are names, a sequence shorter than adapter_k (an
 * empty line too) is ignored and counted in *n_short, a trailing CR is not stripped; every kept sequence s gives the
 * entries s and revcomp(s) (src/utils.cpp:98-129; a byte it DIEs on is KC_ERR_BAD_BASE), and every k-mer of every
 * entry is indexed with Kmer<32>::get_kmers' 2-bit code (N counts as G, nothing is canonicalised).
 * *n_adapters = kept sequences, *n_entries = 2 * *n_adapters, *n_kmers = distinct k-mers (what the reference logs at
 * :132).  adapter_k > 32 is KC_ERR_UNSUPPORTED_K (MAX_ADAPTER_K, src/adapters.hpp:56); a sequence longer than 1024
 * bytes or more than 32768 kept sequences are KC_ERR_INVALID_ARG.  Any output pointer may be NULL.
 */
int kc_adapters_index(const char *text, uint64_t len, int adapter_k, uint64_t *n_adapters, uint64_t *n_short, uint64_t *n_entries,
                      uint64_t *n_kmers);

#define KC_ADAPTERS_BLASTN_SCORES 1u /* align with 2/3/5/2/1 (BLASTN_ALN_SCORES) instead of 1/1/1/1/1: the reference's
                                      * use_blastn_scores, optimize_for == "contiguity" (src/main.cpp:214) */

/*
 * Load an adapter set into the context: the Adapters constructor plus load_adapter_seqs (src/adapters.cpp:48-156).
 * The entries, the k-mer index and the record lists are built on the host as kc_adapters_index builds them (same
 * statuses and counts) and placed in device memory the context owns.  adapter_k = 0: the context's k.  Loading again
 * replaces the set, kc_adapters_clear drops it, kc_reset keeps it (a multi-k sweep trims with the same adapters),
 * kc_destroy frees it.  The set is independent of the table's state: both calls are allowed in any state.
 */
int kc_adapters_load(kc_ctx *ctx, const char *text, uint64_t len, int adapter_k, uint32_t flags, uint64_t *n_adapters,
                     uint64_t *n_short, uint64_t *n_entries, uint64_t *n_kmers);
int kc_adapters_clear(kc_ctx *ctx);

/* Counters of kc_trim_adapters, the reference's (Adapters::done, src/adapters.cpp:158-169) */
typedef struct kc_trim_stats {
  uint64_t reads;         /* reads submitted */
  uint64_t trimmed;       /* reads for which Adapters::trim returned true (a cut of no base included) */
  uint64_t bases_trimmed; /* bases_trimmed: bases cut by trim itself (not by the pair rule) */
  uint64_t reads_removed; /* reads_removed: reads cut to nothing */
  uint64_t alignments;    /* aligner calls (the population of trim_timer_ssw) */
  uint64_t out_bases;     /* bases written */
} kc_trim_stats;

#define KC_TRIM_PAIRED 1u /* reads 2p and 2p+1 are mates: Adapters::trim_pair; without it Adapters::trim per read */

/*
 * Adapter trimming on the device: Adapters::trim_pair (src/adapters.cpp:260-273), the first step of merge_reads' pair
 * loop (src/merge_reads.cpp:469), or with flags = 0 Adapters::trim per read (src/packed_reads.cpp:390), in the build
 * the reference ships (MERGE_READS_TRIM_WITH_SSW).  The exact rules are in csrc/kc_trim.hpp's header comment.
 * Input: interleaved ASCII reads in kc_fastq_pairs' layout (nreads reads, offsets of nreads + 1 entries); device
 * memory (on_device = 1) or host memory, which is staged.  KC_TRIM_PAIRED with an odd nreads is KC_ERR_INVALID_ARG.
 * Output, always device memory, in the same layout with the same number of reads, ready for kc_merge_pairs or
 * kc_submit_reads: a read cut to nothing stays as an empty read.  d_out_bases and d_out_quals hold capacity bytes
 * each, d_out_offsets nreads + 1 entries.  Output bytes never exceed input bytes.
 * KC_ERR_CAPACITY: the arrays are too small (or NULL); *nbytes and *stats hold the totals.  KC_ERR_STATE: no adapter
 * set is loaded (the call is never a silent copy).  KC_ERR_INVALID_ARG: a read longer than 32767.  Base and quality
 * bytes are not validated: the reference's trim looks at no quality, and any byte has a k-mer code and an aligner code.
 * The context's table and state are not touched.  The call runs on the context's stream and returns when its work
 * there is done.
 */
int kc_trim_adapters(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads, int on_device,
                     uint32_t flags, uint8_t *d_out_bases, uint8_t *d_out_quals, uint64_t capacity, uint64_t *d_out_offsets,
                     uint64_t *nbytes, kc_trim_stats *stats);

/*
 * ParseAndPackGPUDriver::process_seq_block input format
 * (src/kcount/kcount_gpu.cpp:167-180, parse_and_pack.cpp:281-319): reads already
 * case-masked (lowercase = low quality) and joined by '_'.
 */
int kc_submit_seq_block(kc_ctx *ctx, const char *seqs, uint64_t len, int on_device);

/*
 * Sharded flow, sender side: extract k-mer records from a block of reads and
 * bin them by owner shard (replaces parse_and_pack + build_supermers + the
 * per-supermer ThreeTierAggrStore::update of kmer_dht.cpp:247-250).  Records of
 * shard d land in d_records[d*seg_capacity*L ...] with L = kc_record_longs(k); h_counts[d] receives
 * how many.  A record is L words: the canonical k-mer with the two
 * extension codes in the low 6 bits of its last word (left | right<<3; 0-3 =
 * ACGT, 4 = none).  KC_ERR_CAPACITY if a segment would overflow (nothing is lost:
 * the table is untouched, call again with more room).
 * Contexts created with KC_FLAG_WIRE_UNITS: records, counts and capacities are UNITS in PIECES, and h_counts has an entry
 * per piece -- see kc_wire_unit below.
 */
int kc_extract_partition(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets,
                         uint64_t nreads, int on_device, uint64_t *d_records, uint64_t seg_capacity,
                         uint64_t *h_counts);
/* The same for a '_'-joined, case-masked block (the format ParseAndPackGPUDriver::process_seq_block takes). */
int kc_extract_partition_seq_block(kc_ctx *ctx, const char *seqs, uint64_t len, int on_device, uint64_t *d_records,
                                   uint64_t seg_capacity, uint64_t *h_counts);
/* Receiver side: HashTableGPUDriver::insert_supermer/insert_supermer_block
 * (gpu_hash_table.cpp:655-695) for records that arrived from other shards. */
int kc_insert_records(kc_ctx *ctx, const uint64_t *d_records, uint64_t n);

/* What kc_extract_partition writes and kc_insert_records reads, for contexts created with KC_FLAG_WIRE_UNITS: a unit is
 * *unit_words words holding *unit_records records, and every destination shard gets *pieces pieces: h_counts has
 * rank_n * *pieces entries, piece j = d * *pieces + q of destination d starts at d_records + j * seg_capacity *
 * *unit_words and holds h_counts[j] units; seg_capacity counts the units of ONE piece (a block of R reads of length L
 * needs about R * (L - k - 1) / (rank_n * *pieces * *unit_records) * 1.3 + 4096); kc_insert_records takes units, a piece
 * or any number of pieces laid end to end, in any order.  Where level 1 writes six-byte records (k = 21 with 1024
 * level-1 buckets) a unit is three words = four records of six bytes -- the k-mer travels mixed, as level 1 stages it,
 * so the receiver neither unpacks nor hashes it; a piece is closed to whole units with marker slots -- and the pieces
 * of a destination hold its records by the top bits of their level-1 bucket (2 to 16 pieces, 128 per sender at most),
 * which is what makes the receiver's level 1 cheap: a round of its 1024-way split that reads out of one piece meets a
 * sixteenth of the buckets and appends sixteen times as much to each.  Otherwise (and without the flag) a unit is one
 * k-mer record of kc_record_longs words and a destination has one piece.  Units are opaque. */
int kc_wire_unit(kc_ctx *ctx, int *unit_words, int *unit_records, int *pieces);
/* kc_insert_records for several pieces that lie `piece_stride_units` units apart (piece j at d_records + j *
 * piece_stride_units * unit_words, h_units[j] units; empty ones are skipped): what a shard keeps for itself of a block it
 * has extracted -- its own pieces of the send buffer, where they lie.  With wire units one launch takes up to sixteen
 * pieces (a round of a workgroup reads out of one), so that many small pieces do not become many small launches. */
int kc_insert_record_pieces(kc_ctx *ctx, const uint64_t *d_records, uint64_t piece_stride_units, int npieces, const uint64_t *h_units);
/* The shard kc_extract_partition sends a canonical k-mer to (role of KmerDHT::get_kmer_target_rank, kmer_dht.cpp:192-196):
 * kc_owner / kc_owner_reference for k-mer records; eight bits of the mixed k-mer for six-byte wire records (bits only
 * the probe stride of a region table uses, so every shard keeps the whole geometry). */
int kc_partition_owner(kc_ctx *ctx, const uint64_t *kmer_words, int *owner);

/* ---- the single-pass shard flow: a shard owns level-1 BUCKETS --------------------------------------------
 * Same role as kc_extract_partition + kc_insert_records -- the aggregated supermer exchange of
 * ThreeTierAggrStore<Supermer>::update / KmerDHT::flush_updates (src/kcount/kmer_dht.cpp:143-151,247-258) plus the
 * owner's insert_supermer_block (gpu_hash_table.cpp:655-695) -- without their two extra passes over the records: the
 * owner of a k-mer is the owner of the level-1 bucket it falls into (each shard a contiguous range of buckets;
 * kc_shard_owner), so the sender's ordinary level-1 pass has already sorted its records by destination.  What other
 * shards own is copied once into one wire segment per destination; what this shard owns never moves; a received segment
 * is read in place by the owner's level 2.  All shards of an exchange must be created with the same kmer_len,
 * max_kmers_buffered, max_elems, rank_n and tuning (a segment carries a signature; a mismatch is KC_ERR_INVALID_ARG).
 * A pass uses either this flow or the hash-ownership entry points (kc_submit_*, kc_insert_records), not both
 * (KC_ERR_STATE); a context on the global-table path (tuning mode 1, or out of buffer) has only the latter.
 */
/* Sender: count_kmers' loop body for one block of reads (src/kcount/kcount.cpp:71-90) + add_supermer for all of it.
 * d_segments: device buffer of rank_n * seg_words u64; segment d (at d * seg_words) receives what shard d owns,
 * h_words[d] = how many words of it to ship (0 for rank_me and for an empty block).  A block of R reads of length L
 * needs about R * (L - k - 1) / rank_n * kc_record_longs(k) * 1.1 + 1024 words per segment at most -- the compact records
 * of k <= 21 with 1024 level-1 buckets travel as FIVE BYTES each (the segment is sorted by bucket, which is therefore
 * implied: the reference compresses its wire too, as supermers, kmer_dht.cpp:69-100), 5/8 of that; h_words says what the
 * segment really holds.  A segment is opaque to the caller: ship h_words[d] words as they are.  KC_ERR_CAPACITY when a segment is
 * too small (the block's k-mers then stay buffered in this context; nothing was shipped) or when the context would
 * hold more than max_kmers_buffered. */
int kc_shard_extract(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads, int on_device,
                     uint64_t *d_segments, uint64_t seg_words, uint64_t *h_words);
/* The same for a '_'-joined, case-masked block (the format ParseAndPackGPUDriver::process_seq_block takes). */
int kc_shard_extract_seq_block(kc_ctx *ctx, const char *seqs, uint64_t len, int on_device, uint64_t *d_segments, uint64_t seg_words,
                               uint64_t *h_words);
/* Receiver: device memory of the context for `nwords` incoming words (the sum over the senders of one block; the caller
 * receives each sender's segment into its own 2-word-aligned part of it).  It belongs to the context and stays valid
 * until kc_reset / kc_destroy; earlier reservations never move. */
int kc_shard_reserve(kc_ctx *ctx, uint64_t nwords, uint64_t **d_dst);
/* Receiver: a whole segment from one sender has landed at d_segment (inside a kc_shard_reserve area, ordered before
 * the context's stream).  It becomes part of this shard's buckets where it lies -- no copy. */
int kc_shard_commit(kc_ctx *ctx, const uint64_t *d_segment, uint64_t nwords);
/* Distinct k-mers this shard's regions hold in this flow before they start spilling to the global table: the shard
 * builds regions only for the buckets it owns, 1/rank_n of the geometry's (at most 2^20 regions of at most 4096 LDS slots
 * for all shards together).  A caller whose shards expect more than this each should stay with kc_extract_partition +
 * kc_insert_records, where every shard uses the whole geometry. */
int kc_shard_capacity(kc_ctx *ctx, uint64_t *max_distinct);
/* The shard that owns a canonical k-mer in this flow (role of KmerDHT::get_kmer_target_rank, kmer_dht.cpp:192-196).
 * Depends on the context's geometry: ask a context of the exchange, not kc_owner. */
int kc_shard_owner(kc_ctx *ctx, const uint64_t *kmer_words, int *owner);

/* ---- the reference's wire format (runs mixed with unmodified MHM2 ranks) -------------------------------- */
/* kcount_gpu::SupermerInfo (src/kcount/kcount-gpu/parse_and_pack.hpp:50-54), same layout */
typedef struct kc_supermer {
  int32_t target; /* KmerDHT::get_kmer_target_rank of the supermer's k-mers */
  int32_t offset; /* first character in the block: the left neighbour of its first k-mer */
  uint16_t len;   /* characters: its k-mers + k + 1 */
} kc_supermer;
/*
 * ParseAndPackGPUDriver::process_seq_block + pack_seq_block (parse_and_pack.cpp:281-336): the supermers of a '_'-joined,
 * case-masked block with the CPU backend's semantics (SeqBlockInserter::process_seq, kcount_cpu.cpp:73-103: maximal
 * runs of k-mers with both neighbours and one target rank) and the block packed two characters per byte with the
 * reference's nibble codes (parse_and_pack.cpp:196-213).  out: capacity entries (host), *n_out = how many there are
 * (KC_ERR_CAPACITY if more than capacity: nothing else is lost, call again with room); *num_valid_kmers = k-mers
 * covered; packed_out: (len + 1) / 2 bytes (host) or NULL.  The context's rank_n gives the number of targets.
 */
int kc_build_supermers(kc_ctx *ctx, const char *seqs, uint64_t len, int on_device, kc_supermer *out, uint32_t capacity,
                       uint32_t *n_out, uint32_t *num_valid_kmers, uint8_t *packed_out);
/*
 * HashTableGPUDriver::insert_supermer_block (gpu_hash_table.cpp:655-679): 4-bit packed supermers as
 * src/kcount/kcount_gpu.cpp:153-161 cuts them (odd nibbles masked to 0), joined by the byte '_' as
 * HashTableGPUDriver::insert_supermer joins them; unpacked on the device (gpu_unpack_supermer_block's role) and
 * inserted like kc_submit_seq_block.
 */
int kc_submit_packed_supermers(kc_ctx *ctx, const uint8_t *packed, uint64_t len, int on_device);

/* The contig k-mer pass (dead in the proxy; the backend surface is complete with it):
 * HashTableInserter::init_ctg_kmers (kmer_dht.hpp:103, kcount_cpu.cpp:472-475; HashTableGPUDriver::init_ctg_kmers,
 * gpu_hash_table.hpp:158) -- room for max_ctg_kmers distinct contig k-mers.  Call before kc_finalize. */
int kc_begin_ctg_kmers(kc_ctx *ctx, uint64_t max_ctg_kmers);
/* SeqBlockInserter::process_seq(ctg->seq, depth) + insert_supermer in the contig pass (kcount.cpp:129,
 * kcount_cpu.cpp:357-407; insert_supermer_block with depths, gpu_hash_table.cpp:655-695): a '_'-joined block of contigs
 * and, per character, the depth of its contig (the layout of SeqBlockInserterState::depth_block, kcount_gpu.cpp:74-91).
 * kc_finalize then returns what the reference's insert_into_local_hashtable would after inserting the contigs behind
 * the reads: the reads' results, plus the contig k-mers that are not among them, whose occurrences agree on both
 * extensions (both bases) and whose smallest depth is at least max(2, dmin_thres), with that depth as their count
 * (kc_ctg.hpp).
 * KC_ERR_BAD_BASE for a character outside ACGTN anywhere in the block (the reference DIEs), KC_ERR_CAPACITY when more
 * distinct k-mers came than kc_begin_ctg_kmers made room for (the table is never filled beyond three quarters: a block is
 * taken in as many launches as its free room asks for).  A context that is one of several ranks (rank_n > 1) keeps of a
 * block only the k-mers the read path would keep there -- what kc_partition_owner names (its share by the k-mer hash, by
 * the reference's target rank with KC_FLAG_REFERENCE_OWNER, by the wire units' owner bits with KC_FLAG_WIRE_UNITS where the
 * geometry has wire units) or, in the shard flow, the owner of the k-mer's level-1 bucket (kc_shard_owner) -- so every rank may be
 * given every contig, or (like the C++ driver, whose host routes supermers by target) only its own. */
int kc_submit_ctg_block(kc_ctx *ctx, const char *seqs, const uint16_t *depths, uint64_t len, int on_device);
/* The contig pass so far: distinct contig k-mers in its table (what done_ctg_kmer_inserts reports as new inserts,
 * gpu_hash_table.cpp:697-734) and characters submitted.  Either pointer may be null. */
int kc_ctg_stats(kc_ctx *ctx, uint64_t *distinct, uint64_t *positions);

/* KmerDHT::flush_updates -> HashTableInserter::flush_inserts (kmer_dht.cpp:252-258): wait for submitted work. */
int kc_flush(kc_ctx *ctx);

/* HashTableGPUDriver::done_all_inserts + the S7/S8 pass of
 * HashTableInserter::insert_into_local_hashtable (gpu_hash_table.cpp:736-784,
 * kcount_cpu.cpp:523-601): vote, purge, compact.  out may be NULL. */
int kc_finalize(kc_ctx *ctx, kc_result *out);
/* begin_iterate/get_next_entry in bulk: copy the results to host arrays sized from kc_result.n. */
int kc_copy_results(kc_ctx *ctx, uint64_t *keys, uint16_t *counts, uint8_t *left, uint8_t *right);
/* The same results in the shape HashTableGPUDriver hands them to its host (output_keys / output_vals,
 * gpu_hash_table.cpp:776-784, gpu_hash_table.hpp:64-75): keys[n*num_longs] and one 8-byte kc_count_exts per entry
 * (= kcount_gpu::CountExts: uint32 count, int8 left, int8 right), packed on the device and copied once, so that a
 * driver's get_next_entry can point straight into the two arrays.  Either pointer may be NULL. */
typedef struct kc_count_exts {
  uint32_t count;
  int8_t left, right;
  int8_t pad[2];
} kc_count_exts;
int kc_copy_results_entries(kc_ctx *ctx, uint64_t *keys, kc_count_exts *vals);
/*
 * Put the results in key order, on the device: ascending, words 0 .. num_longs-1 compared as unsigned integers, which is
 * the alphabetical order of the k-mer strings.  The reference has no such step -- KmerDHT::dump_kmers walks its hash map
 * as it lies (src/kcount/kmer_dht.cpp:273-297) -- and every consumer that compares, searches or merges dumps sorts
 * them on the host first; this is that sort, where the data already is (csrc/kc_sort.hpp: a stable LSD radix sort of a
 * permutation over the 2k significant key bits, then one gather of keys, counts, left and right).
 * Call after kc_finalize (KC_ERR_STATE before it).  out (may be NULL) receives the arrays as kc_finalize would.
 * kc_result pointers obtained EARLIER are invalid after a successful call: the results move to fresh arrays and the
 * old ones are freed.  kc_finalize called afterwards returns the sorted arrays; kc_copy_results,
 * kc_copy_results_entries and kc_dump_text_device follow the new order; kc_lookup answers as before (its index is
 * rebuilt on the next call).  A second call does no device work; kc_reset clears the sorted state.
 * Failure-atomic: on KC_ERR_OUT_OF_MEMORY or KC_ERR_HIP the unsorted results are intact and still valid.  Scratch
 * (2 x 12 bytes a result, and the digit counters) is allocated for the call and freed.
 * The permutation is 32-bit: 2^32 results or more are KC_ERR_CAPACITY (kc_last_error says so).  No test reaches that
 * size.
 */
int kc_sort_results(kc_ctx *ctx, kc_result *out);
/*
 * KmerDHT::dump_kmers' text (src/kcount/kmer_dht.cpp:284: kmer.to_string() << " " << count << " " << left << " " <<
 * right << "\n"), formatted on the device: entries [first, first + count) of the results, in their current order
 * (kc_sort_results first for a sorted dump; not required), as "<k characters ACGT> <count in decimal> <L> <R>\n" into
 * the device memory d_text.  A line is kmer_len + 5 + digits(count) bytes and its newline.  The chunks of any partition of [0, n),
 * laid end to end, are the text of the whole, so a dump of any size streams through a buffer of the caller's choosing
 * (compression and the file stay with the caller).
 * *nbytes always receives the chunk's exact size.  d_text == NULL: a size query.  capacity smaller than that:
 * KC_ERR_CAPACITY, nothing is written.  first + count > n: KC_ERR_INVALID_ARG.  count == 0: KC_OK, *nbytes = 0.
 * KC_ERR_STATE before kc_finalize.  The table is not touched.  The call runs on the context's stream and returns when
 * its work there is done.
 */
int kc_dump_text_device(kc_ctx *ctx, uint64_t first, uint64_t count, uint8_t *d_text, uint64_t capacity, uint64_t *nbytes);
/*
 * Unitigs from the results, on the device: the maximal paths of the de Bruijn graph over (kmer, count, left, right) in
 * which every step is the unique extension on both sides -- what the reference's traverse_debruijn_graph stage would
 * hand to the next, longer k through the contig pass.  The reference's proxy has that stage commented out
 * (src/contigging.cpp), so the rules are THIS project's own definition (pinned by the
 * host model tests/unitig_model.py); no parity with MetaHipMer's traversal is claimed.  In short: an oriented k-mer links
 * to the k-mer its right extension leads to when that k-mer is among the results, its left extension (seen in the same
 * orientation) names the base shifted out, the two are different k-mers and neither is its own reverse complement; a
 * cycle is cut in front of its smallest k-mer; of a path and its reverse complement the one whose first k-mer is the
 * smaller is written; unitigs are ordered by their first k-mer's key, so the output is one exact byte string.
 * Output, in device memory, in the seq-block format: every unitig followed by '_' (d_seqs, *nbytes bytes);
 * d_offsets[u] = start of unitig u, *n_unitigs + 1 entries, so unitig u has d_offsets[u+1] - d_offsets[u] - 1 bases;
 * d_kmer_sums[u] (may be NULL) = the sum of its k-mers' counts; d_depths (may be NULL) = one value per byte of d_seqs,
 * min(65535, mean count rounded half up) on a unitig's bases and 0 on its separator -- d_seqs and d_depths are what
 * kc_submit_ctg_block(..., on_device = 1) takes.  capacity: bytes d_seqs (and values d_depths) has room for;
 * unitigs_capacity: unitigs the arrays have room for (d_offsets holds unitigs_capacity + 1 entries, d_kmer_sums
 * unitigs_capacity).
 * *n_unitigs, *nbytes and *stats (may be NULL) always receive the totals.  d_seqs or d_offsets NULL: a size query.  Arrays
 * that are too small: KC_ERR_CAPACITY, nothing is written.  KC_ERR_STATE before kc_finalize, and for a context that is
 * one of several ranks (rank_n > 1): links across shards are not followed (kc_last_error says so).  2^31 results or
 * more: KC_ERR_CAPACITY (oriented node ids are 32-bit).  NULL ctx, n_unitigs or nbytes: KC_ERR_INVALID_ARG before any
 * device call.  No results: KC_OK, 0 unitigs.
 * The call first puts the results in key order exactly as kc_sort_results does (unless they already are): kc_result
 * pointers obtained EARLIER are invalid afterwards, as that call documents.  It uses the lookup index and builds it if
 * absent.  The table and the results' contents are not touched.  The call runs on the context's stream and returns when
 * its work there is done.  Scratch (73 bytes a result) lives for the call only.
 */
typedef struct kc_unitig_stats {
  uint64_t kmers;      /* results walked */
  uint64_t unitigs;
  uint64_t singletons; /* unitigs of one k-mer */
  uint64_t circular;   /* cycles cut open */
  uint64_t bases;      /* without separators */
  uint64_t longest;    /* in bases */
} kc_unitig_stats;
int kc_build_unitigs(kc_ctx *ctx, uint8_t *d_seqs, uint64_t capacity, uint16_t *d_depths, uint64_t *d_offsets, uint64_t unitigs_capacity,
                     uint64_t *d_kmer_sums, uint64_t *n_unitigs, uint64_t *nbytes, kc_unitig_stats *stats);
/*
 * A seed index over a block of contigs, kept by the context: the first half of putting the reads back onto the contigs
 * just built -- the role of find_alignments in src/contigging.cpp:150-163, which the reference's proxy has commented out
 * like the traversal before it and for which it holds no code (no klign in src/).  So the rules are THIS project's own
 * definition (pinned by the host model tests/align_model.py); no parity with MetaHipMer's klign is
 * claimed.
 * seqs: a seq block as kc_build_unitigs writes it and kc_submit_ctg_block takes it -- nbytes bytes, every contig
 * followed by '_', upper-case A C G T N only; offsets[0] = 0, offsets[u+1] - 1 = the position of contig u's '_',
 * offsets[n_ctgs] = nbytes; empty contigs are allowed.  on_device != 0: seqs and offsets are device pointers.
 * The seed length is the context's kmer_len.  A window is a contig position whose k characters are all ACGT (an N is not
 * G here); its key is the canonical k-mer; a key is a seed iff exactly one window of the whole block has it and it is
 * not its own reverse complement; every other key is "repeated" and never used.
 * The context keeps its own device copy of block and offsets (the caller's arrays are free afterwards) and a table of
 * 8-byte slots, at most half full: 16 to 32 bytes per byte of the block.  The call replaces an earlier index.
 * KC_ERR_BAD_BASE: a byte outside the alphabet; KC_ERR_INVALID_ARG: offsets that do not match the '_'s, a NULL ctx or
 * offsets; KC_ERR_CAPACITY: 2^31 bytes or more (slots hold 32-bit positions); out of memory.  Each of them leaves an
 * earlier index intact (failure-atomic, as kc_sort_results is).  Works before or after kc_finalize and in a context with
 * rank_n > 1; kc_reset and kc_destroy drop the index, kc_ctg_index_clear does so on request.  *stats may be NULL.
 */
typedef struct kc_ctg_index_stats {
  uint64_t contigs;
  uint64_t bases;    /* without separators */
  uint64_t windows;  /* positions whose k characters are all ACGT */
  uint64_t seeds;    /* keys of exactly one window */
  uint64_t repeated; /* keys of several windows, or their own reverse complement */
} kc_ctg_index_stats;
int kc_ctg_index_build(kc_ctx *ctx, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, int on_device,
                       kc_ctg_index_stats *stats);
int kc_ctg_index_clear(kc_ctx *ctx);
/*
 * Reads onto the indexed contigs by seed hits, every hit checked without gaps -- the second half of the role of
 * find_alignments (src/contigging.cpp:150-163); the rules are this project's own (DESIGN.md section 15,
 * tests/align_model.py); gapped alignment is kc_align_gapped's step behind this one.
 * bases / offsets as for kc_merge_pairs (ASCII, nreads + 1 offsets), no qualities; A C G T in either case are bases,
 * anything else is "no base"; a read has at most KC_ALIGN_MAX_READ_LEN bases.  The windows of a read of length L start
 * at p = 0, s, 2s, ... with p + k <= L (s = seed_space >= 1) and consist of bases only.  A window w whose canonical key
 * is a seed at contig u, window offset j, contig text y gives the candidate (u, orient, d): w = y -> orient 0,
 * d = j - p; w = revcomp(y) -> orient 1, d = j - (L - k - p).  With R' the read (orient 0) or its reverse complement:
 * cstart = max(0, d), cstop = min(len_u, d + L), rstart = cstart - d, rstop = cstop - d, mismatches = the i in
 * [rstart, rstop) where R'[i] is no base, or contig[d + i] is N, or the two differ; seeds = the windows that gave the
 * candidate.  A candidate is emitted iff mismatches <= max_mismatches (0xFFFFFFFF keeps all).
 * alns receives one record per emitted candidate, ordered by read, then (ctg, orient, d) ascending -- one exact byte
 * string; read_first (may be NULL) receives nreads + 1 entries: every read's first record, then the total.
 * on_device applies to bases, offsets, alns and read_first alike (a device alns is 16-byte aligned).
 * *n_alns and *stats (may be NULL) always receive the totals.  alns == NULL: a size query, nothing else is written.
 * capacity (records) too small: KC_ERR_CAPACITY, nothing is written.  No index: KC_ERR_STATE.  seed_space == 0, a NULL
 * ctx or n_alns, or a read over the limit (kc_last_error names it): KC_ERR_INVALID_ARG; the pointer checks come before
 * any device call.  nreads == 0: KC_OK.  Neither the table nor the results are touched.  The call runs on the context's
 * stream and returns when its work there is done.  Scratch (8 bytes a read, and the staged input and output of a host
 * caller) lives for the call only.
 */
#define KC_ALIGN_MAX_READ_LEN 1024
typedef struct kc_read_aln {
  uint32_t read, ctg;
  uint32_t cstart, cstop; /* the contig interval */
  uint16_t rstart, rstop; /* the same interval in R' */
  uint16_t mismatches, seeds;
  uint8_t orient;
  uint8_t pad[7]; /* zero */
} kc_read_aln;
typedef struct kc_align_stats {
  uint64_t reads;
  uint64_t reads_aligned; /* reads with at least one record */
  uint64_t windows;       /* windows looked up: all bases */
  uint64_t seed_hits;     /* ... whose key is a seed */
  uint64_t repeated_hits; /* ... whose key is repeated */
  uint64_t alignments;    /* records */
  uint64_t perfect;       /* mismatches 0, rstart 0, rstop = the read's length */
} kc_align_stats;
int kc_align_reads(kc_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads, int on_device, uint32_t seed_space,
                   uint32_t max_mismatches, kc_read_aln *alns, uint64_t capacity, uint64_t *read_first, uint64_t *n_alns,
                   kc_align_stats *stats);
/*
 * Gapped refinement of kc_align_reads' records: one kc_gap_aln for every kc_read_aln, in the same order -- the role of
 * klign's fallback to SSW.  The step around the dynamic programme is this project's own definition (DESIGN.md section
 * 16, tests/gap_model.py); the dynamic programme is the reference's ssw_align (src/ssw/ssw_core.cpp), all five results
 * of Aligner::Align(report_cigar = false), pinned by tests/golden/gap_ref_alignments.json.
 * bases / offsets / nreads: the reads kc_align_reads saw.  alns: n_alns records as it emits them, in any order, several
 * of one read allowed.  With L the read's length, len_u the contig's and d = cstart - rstart, a record is valid iff
 * read < nreads, ctg < the index's contigs, orient <= 1, cstart < cstop <= len_u, rstart < rstop <= L,
 * cstop - cstart == rstop - rstart, cstart == max(0, d) and cstop == min(len_u, d + L); its mismatches field is not
 * read.  Codes: a read's A C G T in either case are 0..3 and anything else 4, a contig's N is 4; R' is the read
 * (orient 0) or its reverse complement (a code c < 4 becomes 3 - c).
 * out[i].mismatches = the positions of [rstart, rstop) where R' or the contig holds a 4 or the two differ; read, ctg,
 * orient and seeds are copied.  mismatches == 0 without KC_GAP_ALWAYS_DP: the input interval with
 * score = match * (rstop - rstart), kind KC_GAP_EXACT.  Every other record: ssw_align of all of R' against
 * contig[wlo, whi), wlo = max(0, d - pad), whi = min(len_u, d + L + pad), in exact integers with the reference's tie
 * rules; a score > 0 gives cstart = wlo + ref_begin, cstop = wlo + ref_end + 1, rstart = query_begin,
 * rstop = query_end + 1, kind KC_GAP_DP; a score of 0 gives four zeros, kind KC_GAP_NONE.
 * scores: 1 <= match <= 9, mismatch and ambiguity <= 9, 1 <= gap_ext <= gap_open <= 9 (what Aligner::ReBuild(string),
 * src/ssw/ssw.cpp:468-480, can express); pad <= KC_GAP_MAX_PAD; flags: KC_GAP_ALWAYS_DP only.
 * on_device applies to bases, offsets, alns and out alike; device record arrays are 16-byte aligned.
 * KC_ERR_INVALID_ARG: a NULL ctx, scores or out, or scores, pad or flags out of range (kc_last_error names the values):
 * all checked before any device call, the ranges before ctx; a read over KC_ALIGN_MAX_READ_LEN or an invalid record
 * (kc_last_error names the read, or the lowest bad record index).  No index: KC_ERR_STATE.  2^32 records or more (the
 * list of records holds 32-bit indices): KC_ERR_CAPACITY.  For every error, of whichever kind, nothing is written
 * through any pointer: neither out nor *stats.  n_alns == 0: KC_OK with zero statistics.  *stats (may be NULL) is
 * written once, on success, and does not depend on the records' order.  Neither the index, the table nor the results are touched.  The call runs on the
 * context's stream and returns when its work there is done.  Scratch (8 bytes a record, and the staged arrays of a host
 * caller) lives for the call only.  Works before or after kc_finalize and in a context with rank_n > 1.
 */
#define KC_GAP_MAX_PAD 1024
#define KC_GAP_ALWAYS_DP 1u
enum { KC_GAP_EXACT = 0, KC_GAP_DP = 1, KC_GAP_NONE = 2 };
typedef struct kc_aln_scores {
  uint32_t match, mismatch, gap_open, gap_ext, ambiguity; /* penalties as positive numbers */
} kc_aln_scores;
typedef struct kc_gap_aln {
  uint32_t read, ctg;
  uint32_t cstart, cstop; /* the contig interval */
  uint16_t rstart, rstop; /* the interval of R' */
  uint32_t score;
  uint16_t mismatches, seeds; /* of the input record's diagonal */
  uint8_t orient, kind;
  uint8_t pad[2]; /* zero */
} kc_gap_aln;
typedef struct kc_gap_stats {
  uint64_t records;
  uint64_t exact;     /* KC_GAP_EXACT */
  uint64_t dp;        /* KC_GAP_DP */
  uint64_t none;      /* KC_GAP_NONE */
  uint64_t cells;     /* sum of L * (whi - wlo) over the records the dynamic programme ran for */
  uint64_t score_sum; /* over all records */
} kc_gap_stats;
int kc_align_gapped(kc_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads, const kc_read_aln *alns, uint64_t n_alns,
                    int on_device, uint32_t pad, const kc_aln_scores *scores, uint32_t flags, kc_gap_aln *out, kc_gap_stats *stats);
/*
 * What the kept contig index holds: *nbytes the block's bytes (separators included), *n_ctgs its contigs -- the sizes of
 * kc_aln_depths' arrays.  Either pointer may be NULL.  KC_ERR_STATE without an index.
 */
int kc_ctg_index_info(kc_ctx *ctx, uint64_t *nbytes, uint64_t *n_ctgs);
/*
 * Contig depths and insert sizes from kc_align_gapped's records, where the records are: the role of the depths the
 * contig pass is fed and of histogrammer.calculate_insert_size(alns) behind find_alignments (src/contigging.cpp:164).
 * The reference holds no code for either (no Alns, no CtgsDepths, no histogrammer in src/), so the rules below are THIS
 * project's own definition (pinned by the host model tests/depth_model.py); no parity with
 * MetaHipMer is claimed.  All quantities are integers; every output is one exact byte string for a given input.
 *
 * Shared by both calls.  alns: n_alns records as kc_align_gapped writes them, in any order.  With len_u the length of
 * contig u of the kept index, a record is VALID iff ctg < n_ctgs, orient <= 1, kind <= 2 and -- unless kind is
 * KC_GAP_NONE, which needs nothing more -- cstart < cstop <= len_u and rstart < rstop <= KC_ALIGN_MAX_READ_LEN; where a
 * call uses reads, also read < nreads, and where it has their lengths, rstop <= L(read) unless kind is KC_GAP_NONE.  An
 * invalid record is KC_ERR_INVALID_ARG and kc_last_error names the lowest bad index; validation is a pass of its own in
 * front of the first store.  A record PASSES THE FILTER iff kind != KC_GAP_NONE, score >= min_score and
 * cstop - cstart >= min_len.  A read's BEST record: among its records that pass, the greatest score, and among equal
 * scores the lowest record index.
 * on_device applies to all arrays alike; device record arrays (alns, ctgs, pairs) are 16-byte aligned.  No index:
 * KC_ERR_STATE.  2^32 records or more: KC_ERR_CAPACITY.  On every error nothing is written through any pointer.  *stats
 * (may be NULL) is written once, on success.  Both calls work before or after kc_finalize and with rank_n > 1, touch
 * neither the index, the table nor the results, run on the context's stream and return when done; scratch lives for
 * the call only.
 *
 * kc_aln_depths.  A record that passes contributes, with e = edge_clip <= KC_DEPTH_MAX_EDGE,
 * lo = cstart + (cstart > 0 ? e : 0) and hi = cstop - (cstop < len_u ? e : 0): 1 to every contig position in [lo, hi)
 * iff lo < hi (an alignment's ends are its least trusted bases, unless the end is the contig's own).  With
 * KC_DEPTH_BEST_ONLY only every read's best record contributes; then read < nreads is part of validity; without the
 * flag neither nreads nor the read field is read.  depth[j], for every byte j of the block, is the number of
 * contributions covering it (exact in 32 bits; 0 on a separator).
 * depths (may be NULL): uint16_t[nbytes], min(depth[j], 65535) -- the layout of kc_submit_ctg_block's depths; with
 * KC_DEPTH_PER_CONTIG every byte of contig u holds u's mean instead, separators 0.
 * ctgs (may be NULL): kc_ctg_depth[n_ctgs]; covered = bases with depth > 0, min_depth / max_depth over the contig's
 * bases, unsaturated (0 for an empty contig), alns = records that contributed,
 * mean = min(65535, floor((depth_sum + len / 2) / len)), 0 for an empty contig.
 * stats: records = none + filtered + not_best + clipped_away + used.
 * n_alns == 0: KC_OK, all-zero outputs (the arrays are written).  Unknown flags or edge_clip over the limit:
 * KC_ERR_INVALID_ARG, checked in front of ctx (kc_last_error names the values).
 */
#define KC_DEPTH_MAX_EDGE 1024
#define KC_DEPTH_BEST_ONLY 1u
#define KC_DEPTH_PER_CONTIG 2u
typedef struct kc_ctg_depth {
  uint64_t depth_sum;
  uint32_t len, covered, min_depth, max_depth, alns, mean;
} kc_ctg_depth;
typedef struct kc_depth_stats {
  uint64_t records;
  uint64_t none;          /* kind KC_GAP_NONE */
  uint64_t filtered;      /* below min_score or min_len */
  uint64_t not_best;      /* only with KC_DEPTH_BEST_ONLY */
  uint64_t clipped_away;  /* passed, but lo >= hi */
  uint64_t used;
  uint64_t bases_covered; /* depth > 0 */
  uint64_t depth_sum;
  uint64_t saturated;     /* bytes whose depth exceeds 65535 */
} kc_depth_stats;
int kc_aln_depths(kc_ctx *ctx, const kc_gap_aln *alns, uint64_t n_alns, uint64_t nreads, int on_device, uint32_t min_score, uint32_t min_len,
                  uint32_t edge_clip, uint32_t flags, uint16_t *depths, kc_ctg_depth *ctgs, kc_depth_stats *stats);
/*
 * kc_pair_inserts.  Reads 2p and 2p + 1 are mates (KC_TRIM_PAIRED's convention); an odd nreads is KC_ERR_INVALID_ARG, as
 * is max_insert outside 1 .. KC_INSERT_MAX (both checked in front of ctx).  offsets: the reads' nreads + 1 offsets (no
 * bases are needed); a read over KC_ALIGN_MAX_READ_LEN is refused as in kc_align_gapped.  Validity includes
 * read < nreads and rstop <= L(read).  With b0, b1 the mates' best records the class of pair p is the first that applies:
 * KC_PAIR_NONE: neither mate has one; KC_PAIR_ONE: exactly one has; KC_PAIR_DIFF_CTG: b0.ctg != b1.ctg;
 * KC_PAIR_SAME_ORIENT: b0.orient == b1.orient; otherwise, with F the orient-0 record, R the orient-1 record and L_R the
 * length of R's read, in signed 64-bit: fs = F.cstart - F.rstart, rs = R.cstart - R.rstart,
 * re = R.cstop + (L_R - R.rstop); KC_PAIR_EVERTED iff rs < fs; else insert = re - fs (at least 1) and KC_PAIR_PROPER iff
 * insert <= max_insert, else KC_PAIR_TOO_LONG.
 * hist (may be NULL): uint64_t[max_insert + 1], hist[i] = the proper pairs with insert i.  pairs (may be NULL):
 * kc_pair_rec[nreads / 2]; aln0 / aln1 the indices of the best records (0xFFFFFFFF: none), insert for PROPER and
 * TOO_LONG, else 0.  stats: insert_sum and insert_sq_sum over the proper pairs; mean and deviation are the caller's.
 */
#define KC_INSERT_MAX 65535
enum { KC_PAIR_NONE = 0, KC_PAIR_ONE = 1, KC_PAIR_DIFF_CTG = 2, KC_PAIR_SAME_ORIENT = 3, KC_PAIR_EVERTED = 4, KC_PAIR_TOO_LONG = 5,
       KC_PAIR_PROPER = 6 };
typedef struct kc_pair_rec {
  uint32_t aln0, aln1;
  uint32_t insert;
  uint8_t cls;
  uint8_t pad[3]; /* zero */
} kc_pair_rec;
typedef struct kc_insert_stats {
  uint64_t pairs;
  uint64_t cls[7]; /* by KC_PAIR_* */
  uint64_t insert_sum, insert_sq_sum;
  uint64_t reads_with_best;
} kc_insert_stats;
int kc_pair_inserts(kc_ctx *ctx, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns, int on_device,
                    uint32_t min_score, uint32_t min_len, uint32_t max_insert, uint64_t *hist, kc_pair_rec *pairs, kc_insert_stats *stats);
/*
 * Contig ends extended by local assembly: the role of localassm(LASSM_MAX_KMER_LEN, kmer_len, packed_reads_list, ins_avg,
 * ins_stddev, qual_offset, ctgs, alns), src/contigging.cpp:167-172, commented out in the proxy.  The reference holds no
 * code for it (no localassm in src/), so the rules below are THIS project's own definition (pinned
 * by the host model tests/lassm_model.py); no parity with MetaHipMer is claimed.  All quantities are integers; every
 * output is one exact byte string for a given input, whatever order the waves or the atomics arrive in.
 *
 * Input.  The reads (bases, quals, offsets as kc_align_gapped takes them; reads 2p and 2p + 1 are mates, an odd nreads is
 * KC_ERR_INVALID_ARG; a read over KC_ALIGN_MAX_READ_LEN is refused as in kc_align_gapped), kc_align_gapped's records
 * alns, kc_pair_inserts' records pairs (nreads / 2 of them) and, optionally, kc_aln_depths' records ctgs (NULL: depth 0
 * for every contig); the contigs are the kept index's.  quals == NULL: every base is high quality; the quality offset is
 * the context's.  alns are valid by the rule above, with read < nreads and rstop <= L(read).  A pairs record is valid iff
 * each of aln0 / aln1 is 0xFFFFFFFF, or is below n_alns with that record's read equal to 2p / 2p + 1 and its kind not
 * KC_GAP_NONE; cls and insert are not read.  An invalid record is KC_ERR_INVALID_ARG and kc_last_error names the lowest
 * bad index; validation is a pass of its own in front of the first store.
 *
 * Codes.  A read's A C G T in either case are 0..3, anything else is 4; a contig's N is 4.  The reverse complement maps
 * c < 4 to 3 - c, keeps 4, and reverses the qualities with the text.  With q = a base's quality byte minus the offset
 * its CLASS is hi iff q >= hi_qual, lo iff min_qual <= q < hi_qual, otherwise none.
 *
 * Ends and candidates.  End 2u is the left end of contig u, end 2u + 1 its right end.  Every walk runs rightwards: a left
 * end is the right end of the contig's reverse complement.  Read r has length L > 0 and a best record b (from pairs);
 * u = b.ctg, R' is the read in contig orientation (its reverse complement iff b.orient is 1), and in signed 64-bit
 * ps = b.cstart - b.rstart, pe = b.cstop + (L - b.rstop).  pe > len_u makes R' a candidate of u's right end; ps < 0
 * makes revcomp(R') a candidate of u's left end.  The mate m = r ^ 1 is UNPLACED FOR u iff its length is > 0 and it has no
 * best record or its best record's contig is not u.  An unplaced m with b.orient == 0 and ps + max_insert > len_u makes
 * revcomp(m) a candidate of u's right end; an unplaced m with b.orient == 1 and pe - max_insert < 0 makes revcomp(m) a
 * candidate of u's left end.  cands counts an end's candidates; an end with none is KC_LASSM_NO_CANDS, one with more
 * than max_cands KC_LASSM_TOO_MANY; either has ext_len, iters and mer_len 0.
 *
 * The table of an end at mer length m.  For every candidate text T of length n and every p with p + m < n: if the window
 * T[p, p + m) is all bases and e = T[p + m] is a base whose class is not none, hi[window][e] or lo[window][e] goes up by
 * one.  Counts are exact.
 *
 * One walk step.  thr = max(min_viable, viable_permille * ctgs[u].mean / 1000) by integer division.  S is the end's tail
 * -- the last min(len_u, max_mer_len) codes of the contig in walk orientation -- followed by the extension so far.  The
 * step yields DEAD_END if |S| < m, or the current mer M (the last m of S) holds a 4, or has no counts; LOOP if M was
 * already visited in this iteration; otherwise M is marked visited and base b is VIABLE iff hi_b + lo_b >= thr and
 * hi_b >= 1: no viable base yields DEAD_END, two or more FORK, exactly one is appended -- and then MAX_LEN is reached iff
 * the extension has max_walk_len bases, else the next step is taken.
 *
 * Iterations.  m starts at min(max(k, min_mer_len), max_mer_len), k the context's kmer_len.  The extension persists across
 * iterations; the table and the visited marks do not.  After FORK, if the last shift was not downward and
 * m + shift <= max_mer_len: m += shift and the next iteration starts.  After DEAD_END, if the last shift was not upward
 * and m - shift >= min_mer_len: m -= shift and the next iteration starts.  Everything else ends the end with that status,
 * the final m in mer_len and the number of iterations in iters.
 *
 * Output.  Contig u becomes revcomp(left extension) + the contig's bytes as they are + the right extension + '_';
 * extensions are upper-case A C G T.  seqs_out / offsets_out (n_ctgs + 1 entries) are in the layout kc_ctg_index_build and
 * kc_submit_ctg_block take; ends (2 n_ctgs records) has out_pos = the block position of the extension's first byte, set
 * for ends without an extension too.  offsets_out, ends and stats may be NULL.  stats: ends = 2 n_ctgs, status by
 * KC_LASSM_*, cands_overhang / cands_mate / cand_bases over every end's candidates (TOO_MANY ends included), iterations
 * and ext_bases summed over the ends, ctgs_extended the contigs with at least one extension base.
 *
 * Protocol.  The parameter ranges (see kc_lassm_params), unknown flags and an odd nreads are checked in front of ctx and
 * kc_last_error names the values.  on_device applies to all arrays alike; device record arrays (alns, pairs, ctgs, ends)
 * are 16-byte aligned, device offsets 8-byte.  No index: KC_ERR_STATE.  2^30 reads or more, 2^32 records or more, or a
 * result of 2^31 bytes or more: KC_ERR_CAPACITY.  On every error nothing is written through any pointer, with one
 * exception: when capacity is too small for the block, or seqs_out is NULL (a size query, KC_OK), *nbytes_out and *stats
 * receive the totals and nothing else is written; a non-NULL seqs_out with too small a capacity is KC_ERR_CAPACITY.
 * nbytes_out is required.  The call works before or after kc_finalize and with rank_n > 1, touches neither the index, the
 * table nor the results, runs on the context's stream and returns when done; scratch lives for the call only: 10 bytes a
 * candidate base and 26 a candidate (the oriented text and the entries of every end that walks), 80 to 160 bytes a
 * candidate base for the tables, but only of the ends of one batch (table_budget_mb bounds the tables of a batch; an
 * end over the budget runs alone), 88 + max_walk_len bytes an end and, for host arrays, the inputs' copies and the
 * outputs' staging (8 bytes a read and the reads' bytes among them).  A read gives at most three candidates.  The
 * result does not depend on table_budget_mb.
 */
#define KC_LASSM_MAX_MER_LEN 128
#define KC_LASSM_MAX_WALK 4096
#define KC_LASSM_MAX_CANDS (1u << 20)
enum { KC_LASSM_NO_CANDS = 0, KC_LASSM_TOO_MANY = 1, KC_LASSM_DEAD_END = 2, KC_LASSM_FORK = 3, KC_LASSM_LOOP = 4, KC_LASSM_MAX_LEN = 5 };
typedef struct kc_lassm_params {
  uint32_t min_mer_len, max_mer_len, shift; /* 4 <= min <= max <= 128, 1 <= shift <= 64 */
  uint32_t max_walk_len;                    /* 1 .. KC_LASSM_MAX_WALK */
  uint32_t max_insert;                      /* 1 .. KC_INSERT_MAX: how far a mate may reach */
  uint32_t min_qual, hi_qual;               /* min_qual <= hi_qual <= 93 */
  uint32_t min_viable, viable_permille;     /* min_viable >= 1, permille <= 1000 */
  uint32_t max_cands;                       /* 1 .. KC_LASSM_MAX_CANDS */
  uint32_t table_budget_mb;                 /* 0 = 1024 */
  uint32_t flags;                           /* 0 */
} kc_lassm_params;                          /* 48 bytes */
typedef struct kc_lassm_end {               /* 16 bytes; index 2u = left end of contig u, 2u + 1 = right */
  uint32_t cands, ext_len, out_pos;         /* out_pos: block position of the extension's first byte */
  uint16_t iters;
  uint8_t mer_len, status;
} kc_lassm_end;
typedef struct kc_lassm_stats {
  uint64_t ends, status[6], cands_overhang, cands_mate, cand_bases, iterations, ext_bases, ctgs_extended;
  uint64_t reserved[5]; /* zero: 144 bytes in all */
} kc_lassm_stats;
int kc_local_assm(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads,
                  const kc_gap_aln *alns, uint64_t n_alns, const kc_pair_rec *pairs, const kc_ctg_depth *ctgs, int on_device,
                  const kc_lassm_params *params, uint8_t *seqs_out, uint64_t capacity, uint64_t *offsets_out,
                  kc_lassm_end *ends, uint64_t *nbytes_out, kc_lassm_stats *stats);
/*
 * Links between contig ends from the alignments: the first half of scaffolding, the adjacency list of the contig graph.
 * The reference holds no code for it (no cgraph, no Alns, no scaffolding in src/), so the rules below are THIS project's
 * own definition (pinned by the host model tests/links_model.py); no parity with MetaHipMer is
 * claimed.  All quantities are integers (signed 64-bit where they are compared); the output is one exact byte string for a
 * given input, whatever order the records come in and whatever order the waves or the atomics arrive in.
 *
 * Input.  The reads' nreads + 1 offsets (no bases are needed; reads 2p and 2p + 1 are mates, an odd nreads is
 * KC_ERR_INVALID_ARG; a read over KC_ALIGN_MAX_READ_LEN is refused as in kc_align_gapped), kc_align_gapped's records alns
 * in ANY order, and kc_pair_inserts' nreads / 2 records pairs (NULL: there are no spans); the contigs are the kept
 * index's.  alns are valid by the rule above, with read < nreads and rstop <= L(read); a pairs record is valid by
 * kc_local_assm's rule (cls and insert are not read).  An invalid read, record or pair -- checked in this order -- is
 * KC_ERR_INVALID_ARG and kc_last_error names the lowest bad index; validation is a pass of its own in front of the first
 * store.  A record PASSES iff it passes the filter above with params->min_score and params->min_len.
 *
 * Ends.  End 2u is the left end of contig u, end 2u + 1 its right end, as in kc_local_assm.
 *
 * Splints.  A passing record a of read r (length L) covers [qs, qe) of the read in the read's own direction:
 * [rstart, rstop) for orient 0, [L - rstop, L - rstart) for orient 1.  With u = a.ctg, a LEAVES u through end 2u + 1 with
 * e = len_u - cstop iff orient is 0 and e <= end_slack, and through end 2u with e = cstart iff orient is 1 and
 * e <= end_slack; it ENTERS u through end 2u with e = cstart iff orient is 0 and e <= end_slack, and through end 2u + 1
 * with e = len_u - cstop iff orient is 1 and e <= end_slack.  Every ordered pair (a, b) of passing records of one read
 * with a.ctg != b.ctg, qs_a < qs_b, qe_a < qe_b, a leaving and b entering has gap = (qs_b - qe_a) - e_a - e_b and is a
 * splint candidate between a's leaving end and b's entering end iff -max_overlap <= gap <= max_splint_gap (otherwise it
 * counts in splints_gap_out).  A read with more than max_read_alns passing records gives no splints and counts in
 * reads_over_cap.  The rule is over all ordered pairs, so it does not depend on the records' order, and the reverse
 * complement of a read gives the same candidates.
 *
 * Spans.  Pair p gives a candidate iff pairs is given, both aln0 and aln1 are present and their contigs differ.  A mate
 * with record b and length L points out of its contig u through end 2u + 1 with d = len_u - (b.cstart - b.rstart) for
 * orient 0, and through end 2u with d = b.cstop + (L - b.rstop) for orient 1.  The pair is a span candidate between the two
 * ends with gap = insert_avg - d0 - d1 iff d0 + d1 <= max_insert; otherwise it counts in spans_too_far.  The filter does
 * not apply to the pairs' records: they were chosen by kc_pair_inserts.
 *
 * Links.  Candidates with the same unordered pair of ends are one link.  A link appears TWICE in links, once in each
 * direction (from, to) and (to, from), with the same figures; links is ordered by (from, to) ascending: the adjacency
 * list of the ends.  The fields of a kind (splint / span) with count 0 are 0; the sums are exact.  end_first (may be
 * NULL): 2 n_ctgs + 1 entries, the index of every end's first record and then the total.  *n_links (required): the
 * number of directed records.  stats (may be NULL): reads = nreads; records = none + filtered + passed;
 * links (undirected) = links_splint_only + links_span_only + links_both; ends_linked = the ends with a record.
 *
 * Protocol.  The parameter ranges (see kc_link_params) and an odd nreads are checked in front of ctx and kc_last_error
 * names the values.  on_device applies to all arrays alike; device record arrays (alns, pairs, links) are 16-byte
 * aligned, device offsets and end_first 8-byte.  No index: KC_ERR_STATE.  2^32 records or more, or 2^31 candidates or
 * more: KC_ERR_CAPACITY.  links == NULL is a size query: KC_OK, *n_links and *stats are written and nothing else; a
 * non-NULL links with capacity (in records) below *n_links is KC_ERR_CAPACITY, with *n_links and *stats written and
 * nothing else.  On every other error nothing is written through any pointer.  n_alns == 0: KC_OK, no records and an
 * all-zero end_first.  The call works before or after kc_finalize and with rank_n > 1, touches neither the index, the
 * table nor the results, runs on the context's stream and returns when done; scratch lives for the call only: 20 bytes
 * a read, 8 a pair, 16 a passing record, 52 a candidate (each is sorted once in either direction) and 48 a directed
 * record, beside the inputs' copies and the outputs' staging for host arrays.
 */
typedef struct kc_link_params {
  uint32_t min_score, min_len; /* the filter */
  uint32_t end_slack;          /* <= KC_LINK_MAX_SLACK: how far from a contig's end an alignment may stop and still reach it */
  uint32_t max_overlap;        /* <= KC_LINK_MAX_OVERLAP: a splint gap of -max_overlap .. max_splint_gap is kept */
  uint32_t max_splint_gap;     /* <= KC_LINK_MAX_SLACK */
  uint32_t insert_avg;         /* 1 <= insert_avg <= max_insert <= KC_INSERT_MAX: a span's gap is insert_avg - d0 - d1 */
  uint32_t max_insert;
  uint16_t max_read_alns;      /* 2 .. KC_LINK_MAX_READ_ALNS passing records a read */
  uint16_t flags;              /* 0 */
} kc_link_params;              /* 32 bytes */
#define KC_LINK_MAX_SLACK 1024
#define KC_LINK_MAX_OVERLAP 65535
#define KC_LINK_MAX_READ_ALNS 64
typedef struct kc_ctg_link { /* 48 bytes */
  uint32_t from, to;         /* ends */
  uint32_t splints, spans;   /* supporting candidates of either kind */
  int32_t splint_gap_min, splint_gap_max, span_gap_min, span_gap_max;
  int64_t splint_gap_sum, span_gap_sum;
} kc_ctg_link;
typedef struct kc_link_stats {
  uint64_t reads, reads_over_cap;
  uint64_t records, none, filtered, passed;
  uint64_t splint_cands, splints_gap_out;
  uint64_t span_cands, spans_too_far;
  uint64_t links, links_splint_only, links_span_only, links_both;
  uint64_t ends_linked;
  uint64_t reserved; /* zero: 128 bytes in all */
} kc_link_stats;
int kc_ctg_links(kc_ctx *ctx, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns, const kc_pair_rec *pairs,
                 int on_device, const kc_link_params *params, kc_ctg_link *links, uint64_t capacity, uint64_t *end_first,
                 uint64_t *n_links, kc_link_stats *stats);
/*
 * Scaffolds from the links: the walk over kc_ctg_links' adjacency list, the second half of scaffolding.  The reference
 * holds no code for it (no cgraph, no scaffolding in src/; src/contigging.cpp stops before it), so the rules below are
 * THIS project's own definition (pinned by the host model tests/scaffold_model.py); no parity with
 * MetaHipMer is claimed.  All quantities are integers (signed 64-bit where they are compared); the output is one exact
 * byte string for a given input.
 *
 * Input.  links: n_links kc_ctg_link records exactly as kc_ctg_links writes them; the contigs are the kept index's block
 * (upper-case A C G T N, every contig followed by '_').  A record is VALID iff from and to are below 2 n_ctgs;
 * from >> 1 != to >> 1; splints + spans >= 1; a kind with count 0 has all its fields 0; a kind with count c > 0 has
 * -KC_LINK_MAX_OVERLAP <= min <= max <= KC_INSERT_MAX and c * min <= sum <= c * max; its key (from, to) is strictly above
 * its predecessor's; and the binary search for the first record whose key is not below (to, from) finds that key with the
 * same eight figures.  An invalid record is KC_ERR_INVALID_ARG and kc_last_error names the lowest bad index; validation is
 * a pass of its own whose verdict is read before anything is stored.
 *
 * Ends and nodes.  End 2u is the left end of contig u, 2u + 1 its right end.  An oriented node is v = 2u + s: s = 0 reads
 * the contig as it stands and is left through end 2u + 1, s = 1 reads its reverse complement (A<->T, C<->G, N stays) and
 * is left through end 2u; twin(v) = v ^ 1.  A node is entered through the end that has its own number.
 *
 * Choosing.  A record QUALIFIES iff splints >= min_splints or spans >= min_spans; its support is splints + spans; its
 * gap is the mean of the splint gaps if splints > 0, else of the span gaps, rounded half up: floor((2 sum + c) / (2 c)).
 * best(e) is the qualifying record of end e's row with the greatest (support, splints), on a tie the smallest `to`;
 * second(e) the greatest of the rest.  e is AMBIGUOUS iff second(e) exists and
 * second.support * 1000 > best.support * max_second_permille.  The edge {e, f} is CHOSEN iff best(e).to = f,
 * best(f).to = e and neither end is ambiguous.
 *
 * Verifying.  With A the text of the node left through e and B the text of the node entered through f: gap >= 0 gives
 * join = gap.  gap < 0, o = -gap: o' is tried in the order o, o + 1, o - 1, o + 2, o - 2, ... up to overlap_slack away, only
 * values with 1 <= o' < min(|A|, |B|); the first o' for which the last o' bytes of A equal the first o' bytes of B (a byte
 * that is not A C G T never matches) gives join = -o'.  If none verifies the edge is dropped (overlaps_rejected).
 *
 * Walking.  next(v) is the node entered through the partner of the end v is left through, or none.  The components are
 * simple paths and cycles, none its own twin.  A cycle is cut open in front of (u*, +), u* its smallest contig, the twin
 * cycle behind (u*, -); such a scaffold has KC_SCAF_CIRCULAR set and its closing join is not written.  Of a path and its
 * twin the one whose head has the smaller contig number is emitted, a single contig as (u, +).  Every contig is a member
 * of exactly one scaffold.
 *
 * Text and order.  A scaffold's text is its head's text, then for every further member with join j: j >= 0 gives j 'N'
 * and the member's text, j < 0 the member's text from byte -j on; then '_'.  Scaffolds are ordered by their head's contig
 * number.  2^31 bytes or more: KC_ERR_CAPACITY.
 *
 * Output.  seqs_out (capacity bytes) / offsets_out (n_scaffolds + 1 entries; n_ctgs + 1 always suffice) in the layout
 * kc_ctg_index_build and kc_submit_ctg_block take; scaffolds: n_scaffolds (at most n_ctgs) records; members: exactly
 * n_ctgs records in scaffold order, out_pos = the block position of the first byte of the member's own text that is
 * written (behind its N run, behind the bytes an overlap merges away); ctg_member: n_ctgs entries, a contig's index in
 * members.  *n_scaffolds and *nbytes_out are required; every other output may be NULL.  stats: edges_chosen =
 * edges_joined + overlaps_rejected; ends_not_mutual counts the ends with a best link whose partner's best is another;
 * edges_joined counts a cycle's closing edge; bases = *nbytes_out - *n_scaffolds.
 *
 * Protocol.  The parameter ranges are checked in front of ctx and kc_last_error names the values.  on_device applies to
 * all arrays alike; device record arrays (links, scaffolds, members) are 16-byte aligned, offsets_out 8-byte, ctg_member
 * 4-byte; seqs_out may have any alignment.  No index: KC_ERR_STATE.  seqs_out == NULL is a size query: KC_OK,
 * *n_scaffolds, *nbytes_out and *stats are written and nothing else; a non-NULL seqs_out with capacity below *nbytes_out
 * is KC_ERR_CAPACITY with the same three written.  On every other error nothing is written through any pointer.
 * n_links == 0: every contig is its own scaffold.  The call works before or after kc_finalize and with rank_n > 1, touches
 * neither the index, the table nor the results, runs on the context's stream and returns when done; scratch lives for the
 * call only: 216 bytes a contig and 8 a record, 24 a contig more while the block is written, none per output byte,
 * beside the records' copy and the outputs' staging for host arrays.
 */
typedef struct kc_scaf_params {
  uint32_t min_splints;         /* >= 1 */
  uint32_t min_spans;           /* >= 1 */
  uint32_t max_second_permille; /* <= 1000 */
  uint32_t overlap_slack;       /* <= KC_SCAF_MAX_SLACK */
  uint32_t flags;               /* 0 */
  uint32_t reserved[3];         /* zero */
} kc_scaf_params;               /* 32 bytes */
#define KC_SCAF_MAX_SLACK 64
#define KC_SCAF_CIRCULAR 1u
typedef struct kc_scaffold_rec { /* 32 bytes; the function has the name kc_scaffold */
  uint32_t first_member, n_members;
  uint32_t len;           /* without the separator */
  uint32_t n_bases;       /* from gaps */
  uint32_t overlap_bases; /* merged away */
  uint32_t flags;         /* KC_SCAF_CIRCULAR: a cycle cut open */
  uint32_t reserved[2];   /* zero */
} kc_scaffold_rec;
typedef struct kc_scaf_member { /* 16 bytes */
  uint32_t ctg;
  int32_t join; /* 0 for a head */
  uint32_t out_pos;
  uint8_t orient, reserved[3];
} kc_scaf_member;
typedef struct kc_scaf_stats {
  uint64_t contigs, records, qualifying;
  uint64_t ends_best, ends_ambiguous, ends_not_mutual, edges_chosen;
  uint64_t overlaps_checked, overlaps_rejected, edges_joined;
  uint64_t scaffolds, singletons, circular;
  uint64_t bases, n_bases, overlap_bases, longest;
  uint64_t reserved[3]; /* zero: 160 bytes in all */
} kc_scaf_stats;
int kc_scaffold(kc_ctx *ctx, const kc_ctg_link *links, uint64_t n_links, int on_device, const kc_scaf_params *params, uint8_t *seqs_out,
                uint64_t capacity, uint64_t *offsets_out, kc_scaffold_rec *scaffolds, kc_scaf_member *members, uint32_t *ctg_member,
                uint64_t *n_scaffolds, uint64_t *nbytes_out, kc_scaf_stats *stats);
/* Closing the scaffolds' gaps from splint reads.  A splint -- one read aligned across two contigs -- holds the bases
 * between the two contig ends; where enough splints agree on the distance, the N run of a join becomes their consensus
 * (or the run goes: the contigs abut, or overlap as their text confirms).  The reference holds no gap closing
 * (src/contigging.cpp stops before scaffolding), so the rules below are this project's own definition (DESIGN.md section
 * 21, tests/close_model.py); no parity with MetaHipMer is claimed.  All quantities are integers, signed 64-bit where
 * they are compared; the output is one exact byte string for a given input, whatever order the records come in.
 *
 * Input.  bases / offsets / alns: the reads and their records exactly as kc_ctg_links takes them (nreads may be odd: no
 * pairs are read), with the same validity, the same filter (min_score, min_len) and the same max_read_alns; the contigs
 * are the kept index's.  scaffolds / members: as kc_scaffold writes them; read are first_member, n_members, ctg, orient and
 * join only (flags is copied; out_pos, len, n_bases, overlap_bases are not read).  Valid iff n_scaffolds >= 1, scaffold 0
 * starts at member 0, every scaffold has n_members >= 1 and starts where its predecessor ends, the last ends at n_ctgs;
 * ctg < n_ctgs, orient <= 1, a member's reserved bytes zero, every contig a member exactly once (of two members with one
 * contig the higher index is the bad one), a head's join 0, any other join in [-KC_LINK_MAX_OVERLAP, KC_INSERT_MAX] and a
 * negative join j with -j < min(len of the member before, len of this member).  Otherwise KC_ERR_INVALID_ARG, and
 * kc_last_error names the lowest bad scaffold, or the lowest bad member, index.  The checks run in the order reads,
 * records, scaffolds, members, each a pass whose verdict is read before anything is stored.
 *
 * Joins.  Member m (not a head) follows member m - 1: the node left is 2 ctg(m-1) + orient(m-1), left through end
 * ea = that ^ 1; the node entered is fb = 2 ctg(m) + orient(m) (kc_scaffold's conventions).  m is a GAP JOIN iff
 * join(m) > 0; only gap joins collect candidates.  A circular scaffold's closing join has no member and is not closed.
 *
 * Candidates.  Exactly kc_ctg_links' splint candidates: an ordered pair (a, b) of passing records of one read with
 * leaving end X, entering end Y, slacks e_a, e_b and gap = (qs_b - qe_a) - e_a - e_b in [-max_overlap, max_splint_gap]; a
 * read over max_read_alns gives none (reads_over_cap).  It supports gap join m FORWARD iff (X, Y) = (ea, fb), BACKWARD
 * iff (X, Y) = (fb, ea); every other candidate counts in cands_off_join.  Its segment is the read's bytes
 * [qe_a + e_a, qs_b - e_b) in the read's own direction (gap bytes for gap >= 0); a backward candidate contributes the
 * segment's reverse complement.
 *
 * Choosing.  g* is the gap value with the most of the join's candidates, on a tie the smallest.  The join is closed iff
 * votes(g*) >= min_reads and votes(g*) * 1000 >= cands * min_agree_permille.  No candidates: KC_CLOSE_NO_READS; not closed:
 * KC_CLOSE_WEAK; in both the run stays and new_join = old_join.
 *
 * Closing.  g* > 0, KC_CLOSE_FILLED: column c of the fill is the base with the most votes among the g*-candidates'
 * segments at c; A C G T in either case vote (a backward candidate's byte is complemented first), every other byte does
 * not; a tie goes to the first of A, C, G, T; a column without votes is 'N'; new_join = g* and the fill stands where the
 * run stood.  g* == 0, KC_CLOSE_ABUT: the run goes, new_join = 0.  g* < 0, o = -g*: KC_CLOSE_OVERLAP with new_join = -o
 * iff 1 <= o < min(|A|, |B|) and the last o bytes of the text left equal the first o bytes of the text entered (a byte
 * that is not A C G T never matches); otherwise KC_CLOSE_OVERLAP_REJECTED and the run is kept.
 *
 * Text and order.  kc_scaffold's rule with the new joins, a filled join's fill in place of its 'N'.  Scaffolds and
 * members keep their order and number.  scaffolds_out: first_member, n_members and flags copied, len, n_bases (the N
 * left) and overlap_bases new; members_out: new_join and the new out_pos; closures: one record a member, in member
 * order; offsets_out: n_scaffolds + 1 entries.  fill_pos is the block position of the first fill byte (filled), of the
 * first 'N' (run kept), otherwise of the member's first written byte.  2^31 bytes or more: KC_ERR_CAPACITY.
 * gaps = gaps_no_reads + gaps_weak + filled + abutted + overlapped + overlaps_rejected; cands counts every splint
 * candidate, cands_off_join those that support no gap join.
 *
 * Protocol.  The parameter ranges are checked in front of ctx and kc_last_error names the values.  on_device applies to
 * all arrays alike; device record arrays (alns, scaffolds, members, scaffolds_out, members_out, closures) are 16-byte
 * aligned, offsets and offsets_out 8-byte; bases and seqs_out may have any alignment.  No index: KC_ERR_STATE.
 * seqs_out == NULL is a size query: KC_OK, *nbytes_out and *stats are written and nothing else; a non-NULL seqs_out with
 * capacity below *nbytes_out is KC_ERR_CAPACITY with the same two written.  On every other error nothing is written
 * through any pointer.  Every output except nbytes_out may be NULL.  n_alns == 0 copies the scaffolds: records and
 * members are rewritten, every gap is KC_CLOSE_NO_READS.  The call works before or after kc_finalize and with rank_n > 1,
 * touches neither the index, the table nor the results, runs on the context's stream and returns when done; scratch lives
 * for the call only: 12 bytes a read, 16 a passing record, 16 a candidate on a gap join, 84 a contig, 8 a scaffold and 1
 * a fill byte, beside the copies of host arrays and the outputs' staging for them.
 */
typedef struct kc_close_params {
  uint32_t min_score, min_len; /* kc_ctg_links' filter */
  uint32_t end_slack;          /* <= KC_LINK_MAX_SLACK */
  uint32_t max_overlap;        /* <= KC_LINK_MAX_OVERLAP */
  uint32_t max_splint_gap;     /* <= KC_LINK_MAX_SLACK */
  uint32_t min_reads;          /* >= 1: supporters a closure needs */
  uint32_t min_agree_permille; /* <= 1000: share of a join's candidates that must agree on the gap */
  uint16_t max_read_alns;      /* 2 .. KC_LINK_MAX_READ_ALNS */
  uint16_t flags;              /* 0 */
} kc_close_params;             /* 32 bytes */
enum {
  KC_CLOSE_HEAD = 0,
  KC_CLOSE_NOT_A_GAP = 1, /* old join <= 0, copied */
  KC_CLOSE_NO_READS = 2,
  KC_CLOSE_WEAK = 3,
  KC_CLOSE_FILLED = 4,
  KC_CLOSE_ABUT = 5,
  KC_CLOSE_OVERLAP = 6,
  KC_CLOSE_OVERLAP_REJECTED = 7
};
typedef struct kc_closure { /* 32 bytes, one a member */
  uint32_t cands;           /* the join's candidates */
  uint32_t reads;           /* candidates of the chosen gap; 0 where none was chosen */
  int32_t old_join, new_join;
  uint32_t fill_pos;
  uint32_t disputed; /* fill columns whose voters do not all agree */
  uint8_t status, pad[3];
  uint32_t reserved; /* zero */
} kc_closure;
typedef struct kc_close_stats { /* 128 bytes */
  uint64_t members, joins, gaps;
  uint64_t reads_over_cap, passed, cands, cands_off_join;
  uint64_t gaps_no_reads, gaps_weak, filled, abutted, overlapped, overlaps_rejected;
  uint64_t fill_bases, n_bases_left, disputed_cols;
} kc_close_stats;
int kc_close_gaps(kc_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t nreads, const kc_gap_aln *alns, uint64_t n_alns,
                  const kc_scaffold_rec *scaffolds, uint64_t n_scaffolds, const kc_scaf_member *members, int on_device,
                  const kc_close_params *params, uint8_t *seqs_out, uint64_t capacity, uint64_t *offsets_out, kc_scaffold_rec *scaffolds_out,
                  kc_scaf_member *members_out, kc_closure *closures, uint64_t *nbytes_out, kc_close_stats *stats);
/* The read pairs regrouped by their home contig: the role of shuffle_reads(qual_offset, packed_reads_list, ctgs),
 * src/contigging.cpp:128-147, commented out in the proxy.  The reference holds no code for it (no shuffle_reads in src/),
 * so the rules below are this project's own definition (tests/shuffle_model.py); no parity with
 * MetaHipMer is claimed.  All quantities are integers; every output is one exact byte string for a given input.
 *
 * Input.  Reads 2p and 2p + 1 are mates; bases / quals / offsets: the reads (quals may be NULL, then quals_out is NULL
 * too); alns: kc_align_gapped's records in any order; pairs: kc_pair_inserts' records for these reads and these records.
 *
 * Home.  A pair's candidates are the records its aln0 and aln1 name (0xFFFFFFFF: none).  Without a candidate the pair is
 * HOMELESS and its home is KC_SHUFFLE_NO_HOME.  Otherwise the chosen record is the first by (greater score, smaller ctg,
 * smaller cstart, mate 0 before mate 1); its ctg is the pair's HOME, its cstart the pair's ANCHOR.
 *
 * Order.  Homed pairs are ordered by (home, anchor, old pair index), homeless pairs by old pair index: one stable radix
 * sort of a 32-bit permutation by the key home << b | anchor, b the bit length of the longest contig, a homeless pair with
 * n_ctgs in the home field; the sort runs over the key's key_bits = b + bit length of n_ctgs significant bits only.
 *
 * Parts.  With NH homed and NU homeless pairs, part j of `parts` takes the homed pairs of rank
 * [floor(j NH / parts), floor((j + 1) NH / parts)) and behind them the homeless pairs of rank [floor(j NU / parts),
 * floor((j + 1) NU / parts)); the new order is part 0, part 1, ...  part_starts[j] = floor(j NH / parts) +
 * floor(j NU / parts) for j in [0, parts], so part_starts[parts] = the pairs; a part may be empty.  parts = 1: all homed
 * pairs, then all homeless ones.
 *
 * Output, q a new pair index.  order[q]: the old pair index; home[q]: the pair's home; offsets_out: the nreads + 1 offsets
 * of the reads in new order (mates stay adjacent and keep their order); bases_out / quals_out: the same bytes at the new
 * offsets; alns_out (may be NULL): alns in the same order with `read` rewritten to the read's new index, so that the
 * indices in pairs stay valid; pairs_out (may be NULL): pairs_out[q] = pairs[order[q]]; stats (may be NULL): written
 * once, on success; homed = one_mate + two_same + two_diff, bytes = offsets[nreads].
 *
 * Protocol.  Checked in front of ctx, kc_last_error naming the values, each KC_ERR_INVALID_ARG: an odd nreads; parts
 * outside 1 .. KC_SHUFFLE_MAX_PARTS; a NULL bases_out, offsets_out, order, home or part_starts, or NULL pairs with
 * nreads > 0; quals and quals_out not both NULL or both given; an output that is an input array.  on_device applies to all
 * arrays alike; device record arrays (alns, pairs, alns_out, pairs_out) are 16-byte aligned, offsets, offsets_out and
 * part_starts 8-byte, order and home 4-byte; bases, quals and their outputs may have any alignment.  No index:
 * KC_ERR_STATE.  2^32 reads or records, or more: KC_ERR_CAPACITY.  A read over KC_ALIGN_MAX_READ_LEN or decreasing
 * offsets, an invalid record (kc_pair_inserts' validity), a pair that names a record out of range, of another read or of
 * kind KC_GAP_NONE: KC_ERR_INVALID_ARG, kc_last_error names the lowest bad index; the checks run in the order reads,
 * records, pairs, each a pass whose verdict is read before anything is stored, so on every error nothing is written
 * through any pointer.  nreads == 0: KC_OK, offsets_out[0] = 0, part_starts all 0.  The call works before or after
 * kc_finalize and with rank_n > 1, touches neither the index, the table nor the results, runs on the context's stream
 * and returns when done; scratch lives for the call only: 36 bytes a pair, 8 a read and 4 for every 4096 bytes of the reads, beside the copies of host arrays
 * and the outputs' staging for them.
 */
#define KC_SHUFFLE_MAX_PARTS 65536
#define KC_SHUFFLE_NO_HOME 0xFFFFFFFFu
typedef struct kc_shuffle_stats { /* 80 bytes */
  uint64_t pairs, homed, homeless;
  uint64_t one_mate;       /* homed through the only mate that has a best record */
  uint64_t two_same;       /* both mates have one, on the same contig */
  uint64_t two_diff;       /* both have one, on different contigs */
  uint64_t homes;          /* distinct contigs that are some pair's home */
  uint64_t max_home_pairs; /* the pairs of the home that has the most */
  uint64_t bytes;          /* offsets[nreads] */
  uint64_t key_bits;       /* significant bits the sort ran over */
} kc_shuffle_stats;
int kc_shuffle_reads(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads,
                     const kc_gap_aln *alns, uint64_t n_alns, const kc_pair_rec *pairs, int on_device, uint32_t parts,
                     uint8_t *bases_out, uint8_t *quals_out, uint64_t *offsets_out, uint32_t *order, uint32_t *home,
                     uint64_t *part_starts, kc_gap_aln *alns_out, kc_pair_rec *pairs_out, kc_shuffle_stats *stats);
/* The end of the assembly: which contigs are printed, in which order, the figures everybody quotes, and the FASTA text.
 * The roles of ctgs.dump_contigs(fname, min_ctg_print_len, prefix), src/main.cpp:262 and src/contigging.cpp:115,180, and of
 * ctgs.print_stats(min_ctg_len), src/contigging.cpp:184 and src/main.cpp:266, all commented out in the proxy.  The
 * reference holds no Contigs class, so the rules below are this project's own definition (DESIGN.md section 23,
 * tests/asm_model.py); no parity with MetaHipMer is claimed.  All quantities are integers; every output is one exact byte
 * string for a given input.
 *
 * Both calls take a seq block exactly as kc_ctg_index_build takes it: seqs / nbytes / offsets / n_ctgs, every contig
 * followed by '_', upper-case A C G T N, offsets[0] = 0, offsets[n_ctgs] = nbytes; empty contigs are allowed; 2^31 bytes
 * or more: KC_ERR_CAPACITY.  on_device applies to all arrays of a call alike (params is always the host's); device
 * offsets are 8-byte aligned, order 4-byte, seqs and text may have any alignment.  Neither call needs the contig index,
 * the table or the results; both work before or after kc_finalize and with rank_n > 1, run on the context's stream,
 * return when their work is done, keep no state in the context and free their scratch with the call.  The ranges of the
 * parameters are checked in front of ctx, kc_last_error naming the values.  On every error nothing is written through
 * any pointer.
 *
 * kc_ctg_select.  A contig is SELECTED iff its length, without the separator, is >= min_len.  order (may be NULL; room
 * for n_ctgs entries, of which the first *n_selected are written) receives the selected contigs' block indices: in block
 * order, or with KC_ASM_BY_LENGTH by length, longest first, equal lengths by smaller index first.  Unknown flags or
 * non-zero reserved words: KC_ERR_INVALID_ARG.  The block is checked as kc_ctg_index_build checks it, with the same
 * verdicts (KC_ERR_BAD_BASE; KC_ERR_INVALID_ARG for offsets that do not match the separators), read before anything is
 * stored.  *n_selected and *stats (may be NULL) are always written on success.
 *
 * Statistics.  contigs, bases: the whole block, without separators.  selected, sel_bases; a, c, g, t, n: byte counts
 * over the selected contigs.  n_runs: positions p of a selected contig with seqs[p] == 'N' and (p == 0 or
 * seqs[p - 1] != 'N'): a run that ends one contig and a run that begins the next are two runs, the '_' between them is
 * not N.  longest, shortest: over the selected contigs, both 0 without any.  With the selected lengths in descending
 * order l_1 >= l_2 >= ..., their prefix sums S_i and total T: Lx is the smallest i with 100 S_i >= x T, Nx = l_Lx, both 0
 * when nothing is selected (n50, l50, n90, l90).  ge_count[j], ge_bases[j]: the selected contigs of length >=
 * KC_ASM_CLASSES[j] and their bases.  key_bits: the significant bits the sort ran over, those of longest - shortest (the
 * sort is a stable radix sort of a 32-bit permutation by the key longest - length; it always runs, Nx needs it).
 * Scratch: 45 bytes a contig and 4 for every 4096 bytes of the block, beside the copies of host arrays.
 *
 * kc_fasta_text.  line_width is 0 or 1 .. 65535, prefix_len at most KC_FASTA_MAX_PREFIX, every prefix byte 0x21 .. 0x7E,
 * flags and the reserved words zero; written and total are required.  order == NULL: all contigs in block order, n_order
 * must then equal n_ctgs; entries may repeat; an entry >= n_ctgs is KC_ERR_INVALID_ARG and kc_last_error names the lowest
 * bad index.  The offsets are checked contig by contig (offsets[0] == 0, strictly increasing, offsets[n_ctgs] == nbytes,
 * a '_' in front of each): KC_ERR_INVALID_ARG.  The alphabet is NOT checked, that is kc_ctg_select's job: bytes are
 * copied as they are.
 *
 * The text.  For j = 0 .. n_order - 1, u = order[j]: '>' prefix u-in-decimal '\n', then the contig's bytes in lines of
 * line_width, each followed by '\n'; line_width 0: one line.  max(1, ceil(len / line_width)) lines: an empty contig gives
 * one empty line.  A record is 1 + prefix_len + digits(u) + 1 + len + lines bytes.  line_width 0 with the prefix
 * "scaffold_" is dump_contigs' format.
 *
 * The window.  The call writes bytes [first_byte, min(total, first_byte + capacity)) of the whole text to text; *written
 * receives the window's size, *total the size of the whole text, on every success.  text == NULL: a size query, 0 written.
 * first_byte > total: KC_ERR_INVALID_ARG (kc_last_error names the total); first_byte == total: KC_OK, 0 written.  The
 * windows of any partition of [0, total), laid end to end, are the whole text: a text of any size streams through a
 * buffer of the caller's choosing, whatever the longest contig.  The records' starts are recomputed on every call, at 8
 * bytes (scratch and traffic) per order entry, so choose windows far larger than that: megabytes, not records.
 */
#define KC_ASM_BY_LENGTH 1u
#define KC_ASM_CLASSES {1000u, 5000u, 10000u, 25000u, 50000u}
#define KC_FASTA_MAX_PREFIX 32
typedef struct kc_asm_params { /* 32 bytes */
  uint32_t min_len;
  uint32_t flags;
  uint32_t reserved[6]; /* zero */
} kc_asm_params;
typedef struct kc_asm_stats { /* 256 bytes */
  uint64_t contigs, bases;
  uint64_t selected, sel_bases;
  uint64_t a, c, g, t, n;
  uint64_t n_runs;
  uint64_t longest, shortest;
  uint64_t n50, l50, n90, l90;
  uint64_t ge_count[5], ge_bases[5];
  uint64_t key_bits;
  uint64_t reserved[5]; /* zero */
} kc_asm_stats;
typedef struct kc_fasta_params { /* 64 bytes */
  uint32_t line_width, prefix_len, flags, reserved0;
  char prefix[32];
  uint32_t reserved[4]; /* zero */
} kc_fasta_params;
int kc_ctg_select(kc_ctx *ctx, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, int on_device,
                  const kc_asm_params *params, uint32_t *order, uint64_t *n_selected, kc_asm_stats *stats);
int kc_fasta_text(kc_ctx *ctx, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, const uint32_t *order,
                  uint64_t n_order, int on_device, const kc_fasta_params *params, uint64_t first_byte, uint8_t *text, uint64_t capacity,
                  uint64_t *written, uint64_t *total);
/* FASTA text -> a seq block, on the device: the inverse of kc_fasta_text, and the contig side's twin of
 * kc_fastq_to_packed_device.  It takes up what dump_contigs / --checkpoint wrote (src/contigging.cpp:82,115,177-180,
 * src/main.cpp:262), or somebody else's assembly: line-wrapped, lower-case, IUPAC codes, CRLF.  The reference holds no
 * Contigs::load_contigs, so the rules below are this project's own definition (DESIGN.md section 24,
 * tests/fasta_in_model.py); no parity with MetaHipMer is claimed.  All quantities are integers; every output is one exact
 * byte string for a given input.
 *
 * Lines, as in kc_fastq_to_packed: a line ends at '\n', the last line may lack it.  Trailing '\r', ' ' and '\t' are not part
 * of a line.  Positions in the text are 64-bit; a text may exceed 2^32 bytes.
 *
 * Records.  A line whose first byte is '>' is a header and begins a record.  Empty lines (after stripping) are ignored
 * everywhere.  A record's sequence is the concatenation of its non-header lines up to the next header or the end of the
 * text.  A header with no sequence gives an empty contig.  A non-empty non-header line in front of the first header is a
 * structural error; its position is that of its first byte.
 *
 * Alphabet: kc_fastq_to_packed's table (PackedRead, src/packed_reads.cpp:99-124).  A C G T are copied as they are, a c g t
 * become upper case, N n U R Y K M S W B D H V become N.  Every other byte inside a sequence line is a bad base; interior
 * white space counts.  With KC_FASTA_STRICT everything but A C G T N is a bad base.
 *
 * Errors.  The error at the smallest text position wins, whichever kind it is (at one position, the structural one).  A
 * sequence before the first header: KC_ERR_INVALID_ARG, kc_last_error "fasta: line L: sequence before the first header".
 * A bad base: KC_ERR_BAD_BASE, kc_last_error "fasta: line L column C: byte 0xHH is not a base".  L and C are 1-based, C
 * counts bytes from the line's start.  A format error wins over KC_ERR_CAPACITY.  On every error nothing is written through
 * any output pointer: the validation runs before any store to the caller's arrays.
 *
 * Output.  seqs: the block, *nbytes bytes, every contig followed by '_' (room for seqs_capacity bytes).  offsets:
 * *n_ctgs + 1 entries, offsets[0] = 0 (room for ctgs_capacity + 1).  depths (may be NULL; room for seqs_capacity entries):
 * one uint16 per byte of the block, the record's depth on its bases and 0 on its separator, exactly what
 * kc_submit_ctg_block(..., on_device = 1) takes.  recs (may be NULL; room for ctgs_capacity): one kc_fasta_rec per contig.
 * A block of 2^31 bytes or more is KC_ERR_CAPACITY, as every consumer of a block says.  NULL seqs or offsets is a size
 * query: KC_OK, nothing written but the totals.  Arrays that are too small: KC_ERR_CAPACITY, nothing written but the
 * totals.  *n_ctgs, *nbytes, *consumed (may be NULL) and *stats (may be NULL) receive the totals on success and on
 * KC_ERR_CAPACITY.
 *
 * kc_fasta_rec.  hdr_pos: the text position of the '>'.  hdr_len: the stripped header's length including '>'.  seq_lines:
 * the record's non-empty sequence lines.  flags: KC_FASTA_HAS_ID, KC_FASTA_HAS_DEPTH, KC_FASTA_LOWERED (a byte of acgtn
 * was seen in the record), KC_FASTA_RECODED (a byte of URYKMSWBDHV was seen).  The header parse looks at the first
 * KC_FASTA_HDR_SCAN = 256 bytes of the stripped header only; a token that does not end inside them (at a blank or at the
 * header's end) is absent.  The first token is the run of bytes other than ' ' and '\t' right after '>'.  id is the value
 * of the maximal run of decimal digits at the first token's end, present iff that run has 1 to 18 digits; otherwise id = 0
 * and the flag is clear.  The second token follows the white space.  The depth is present iff the whole second token is 1
 * to 9 digits, optionally followed by '.' and any number of digits: depth = min(65535, integer part + (first fractional
 * digit >= '5')).  Otherwise depth = params->default_depth and the flag is clear.  kc_fasta_text's own ">scaffold_17" gives
 * id 17, so text written by this library comes back with its block indices; MetaHipMer's ">Contig123 17.4" gives id 123,
 * depth 17.
 *
 * KC_FASTA_PARTIAL.  The text is a prefix of a longer input, and only whole records count: a record is whole iff another
 * header begins behind it inside the text.  *consumed is the position of the last '>' at a line's start, 0 when there is
 * none (KC_OK with 0 contigs).  The call equals the flag-free call on text[0, *consumed) in status, outputs, error text
 * and statistics; an error at or behind *consumed is not reported.  Without the flag *consumed = len.  A caller streams a
 * file by carrying the tail into the next call and making the last call without the flag.
 *
 * Parameters: flags, default_depth (0 .. 65535), reserved words zero.  Unknown flags, non-zero reserved words, a
 * default_depth out of range and NULL n_ctgs / nbytes / params are KC_ERR_INVALID_ARG, refused in front of ctx with
 * kc_last_error naming the value.  Statistics: lines, empty_lines (after stripping), records, empty_records, bases (the
 * block without separators), lowered and recoded (bytes of acgtn / of URYKMSWBDHV), longest (contig), with_id, with_depth.
 *
 * on_device = 1: the text is read in place from device memory and all output arrays are device pointers (offsets and recs
 * 8-byte aligned, depths 2-byte; text and seqs may have any alignment).  on_device = 0: the text is host memory, staged in
 * one copy, and the outputs are host arrays.  The call needs neither table, results nor index, works in any state and
 * with rank_n > 1, runs on the context's stream, returns when its work is done, keeps nothing in the context and frees
 * its scratch: 24 bytes a line and 8 a '\n', 52 a record, 8 for every 4096 bytes of text and of block and for every 64 KiB
 * of text, beside the copies of host arrays.
 */
#define KC_FASTA_PARTIAL 1u
#define KC_FASTA_STRICT 2u
#define KC_FASTA_HDR_SCAN 256
#define KC_FASTA_HAS_ID 1u
#define KC_FASTA_HAS_DEPTH 2u
#define KC_FASTA_LOWERED 4u
#define KC_FASTA_RECODED 8u
typedef struct kc_fasta_in_params { /* 32 bytes */
  uint32_t flags;
  uint32_t default_depth;
  uint32_t reserved[6]; /* zero */
} kc_fasta_in_params;
typedef struct kc_fasta_in_stats { /* 128 bytes */
  uint64_t lines, empty_lines;
  uint64_t records, empty_records;
  uint64_t bases, lowered, recoded;
  uint64_t longest;
  uint64_t with_id, with_depth;
  uint64_t reserved[6]; /* zero */
} kc_fasta_in_stats;
typedef struct kc_fasta_rec { /* 32 bytes */
  uint64_t hdr_pos;
  uint32_t hdr_len, seq_lines;
  uint64_t id;
  uint32_t depth, flags;
} kc_fasta_rec;
int kc_fasta_to_block(kc_ctx *ctx, const uint8_t *text, uint64_t len, int on_device, const kc_fasta_in_params *params, uint8_t *seqs,
                      uint64_t seqs_capacity, uint64_t *offsets, uint64_t ctgs_capacity, uint16_t *depths, kc_fasta_rec *recs,
                      uint64_t *n_ctgs, uint64_t *nbytes, uint64_t *consumed, kc_fasta_in_stats *stats);
/* Reads -> FASTQ text, on the device: the inverse of kc_fastq_pairs / kc_fastq_to_packed, and the read side's twin of
 * kc_fasta_text.  It plays the role of merge_reads' --dump-merged hand-over (src/merge_reads.cpp:335-340,379-382,635-647):
 * "@r<id>/1", sequence, "+", qualities.  The reference also writes " #<original name>" behind the name; this library
 * keeps no names, so the rules below are this project's own definition (tests/fastq_out_model.py);
 * no parity with MetaHipMer's files beyond the four-line records and the r<id>/<mate> names is claimed.
 *
 * Input.  The reads lie as everywhere in the front end: read r is [offsets[r], offsets[r + 1]) of bases and of quals,
 * no separators, offsets[0] == 0.  Without KC_FASTQ_OUT_PACKED both arrays are ASCII (kc_fastq_pairs' and
 * kc_shuffle_reads' output).  With it quals must be NULL and bases holds the read cache's byte per base (kc_merge_pairs'
 * and kc_fastq_to_packed's output): the base is "ACGTN"[b & 7], N for the codes 5 to 7, the quality the byte
 * (b >> 3) + qual_offset of the context.  on_device applies to all arrays alike; device offsets and ids are 8-byte
 * aligned, order 4-byte; bases, quals and text may have any alignment.
 *
 * The text.  For j = 0 .. n_order - 1, i = order[j], or i = j when order is NULL (n_order must then equal nreads):
 *   '@' prefix number(i) [ "/1" | "/2" ] '\n' bases '\n' '+' '\n' qualities '\n'
 * number(i) = ids ? ids[i] : first_id + (PAIRED ? i - (i & 1) : i), in decimal: the reference's r0/1 r0/2 r2/1 r2/2 for
 * the prefix "r".  The suffix is there only with KC_FASTQ_OUT_PAIRED and follows the parity of i; order may hold the even
 * reads only, which is how the mate-1 file of a pair of files is written.  Entries of order may repeat.  An empty read
 * gives two empty lines (kc_fastq_pairs takes that).  A record is 6 + prefix_len + digits + (PAIRED ? 2 : 0) + 2 len bytes.
 *
 * The window: kc_fasta_text's contract.  The call writes bytes [first_byte, min(total, first_byte + capacity)) of the whole
 * text to text; *written and *total are set on every success.  text == NULL: a size query.  first_byte > total:
 * KC_ERR_INVALID_ARG (kc_last_error names the total); first_byte == total: KC_OK, 0 written.  The windows of any partition
 * of [0, total), laid end to end, are the whole text.  All positions are 64-bit.  The records' starts are recomputed on
 * every call, at 8 bytes per order entry: choose windows of megabytes.
 *
 * Errors.  On every error nothing is written through any pointer.  In front of ctx, kc_last_error naming the value,
 * KC_ERR_INVALID_ARG: unknown flags, non-zero reserved words, prefix_len > KC_FASTQ_OUT_MAX_PREFIX, a prefix byte outside
 * 0x21 .. 0x7E, PACKED with quals, no PACKED without quals where nreads > 0, NULL written / total / params, order == NULL
 * with n_order != nreads; KC_ERR_CAPACITY: nreads or n_order of 2^32 or more.  Behind ctx and in front of the first
 * store: PAIRED with an odd nreads is KC_ERR_INVALID_ARG; offsets that do not start at 0 or decrease are
 * KC_ERR_INVALID_ARG; a read of 2^32 bytes or more is KC_ERR_CAPACITY; an order[j] >= nreads is KC_ERR_INVALID_ARG and
 * kc_last_error names the lowest such j; a number over 9 999 999 999 999 999 (sixteen digits, what a 64-bit BCD word
 * carries) is KC_ERR_INVALID_ARG, naming the lowest j.
 *
 * KC_FASTQ_OUT_CHECK.  Every base and quality byte of every read that order names (every call checks them all, whatever
 * the window: check with the size query, then stream without the flag) must be 0x21 .. 0x7E in ASCII reads -- the text
 * would not parse back otherwise -- and every code b & 7 must be <= 4 in packed reads.  The first offending byte is
 * KC_ERR_BAD_BASE: first in (j, bases before qualities, position); kc_last_error names j, the read, the position and the
 * byte.  A bad byte in a read that order leaves out is no error.  Without the flag bytes are copied or decoded as they are.
 *
 * The call needs neither table, results nor index, works in any state and with rank_n > 1, runs on the context's stream,
 * returns when its work is done, keeps nothing in the context and frees its scratch: 8 bytes an order entry, with CHECK
 * and an order 4 a read, 4 for every 4096 bytes of the window, beside the copies of host arrays.
 */
#define KC_FASTQ_OUT_PACKED 1u  /* bases holds the read cache's packed bytes, quals is NULL */
#define KC_FASTQ_OUT_PAIRED 2u  /* reads 2p and 2p+1 are mates: names end in "/1" and "/2" */
#define KC_FASTQ_OUT_CHECK  4u  /* validate every byte before the first store */
#define KC_FASTQ_OUT_MAX_PREFIX 32
typedef struct kc_fastq_out_params { /* 64 bytes */
  uint32_t flags, prefix_len;
  uint64_t first_id;
  char prefix[32];
  uint32_t reserved[4]; /* zero */
} kc_fastq_out_params;
int kc_fastq_text(kc_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t nreads,
                  const uint32_t *order, uint64_t n_order, const uint64_t *ids, int on_device,
                  const kc_fastq_out_params *params, uint64_t first_byte, uint8_t *text, uint64_t capacity,
                  uint64_t *written, uint64_t *total);
/* Duplicate and contained contigs of a seq block, removed on the device.  kc_local_assm grows neighbouring contigs towards
 * each other and over the short contigs between them, load_contigs and a second round bring their own copies, and the seed
 * index (kc_ctg_index_build) throws away exactly the k-mers two copies share: reads stop aligning to both.  The reference
 * holds no contig code, so the rules below are this project's own definition (tests/dedup_model.py); no
 * parity with MetaHipMer is claimed.  All quantities are integers; every output is one exact byte string for a given input.
 *
 * Input: a seq block exactly as kc_ctg_index_build takes it (seqs / nbytes / offsets / n_ctgs, every contig followed by '_',
 * upper-case A C G T N, empty contigs allowed, 2^31 bytes or more: KC_ERR_CAPACITY) and, optionally, depths: one uint16 per
 * byte of the block, as kc_submit_ctg_block takes them.  k is the context's kmer_len.
 *
 * Contigs and order.  T_u is contig u's text, L_u its length, rc(T) the reverse complement, N staying N.  v OUTRANKS u iff
 * L_v > L_u, or L_v == L_u and v < u: a strict total order, so the top contig is never removed.
 * Anchor.  a_u is the smallest p for which T_u[p, p + k) is all A C G T.  A contig without one (shorter than k, or dense in
 * N) is UNANCHORED: it is always kept.  It has no window either, so no candidate names it as v: it contains nothing.
 * Window.  A window of v is a position w for which T_v[w, w + k) is all A C G T; it never crosses a '_'.
 * Candidate (u, v, w, o): u is anchored; v != u and v outranks u; w is a window of v; o is 0 or 1 and v's window text equals
 * u's anchor text (o = 0) or its reverse complement (o = 1), a palindromic anchor giving both; and with j = w - a_u (o = 0)
 * or j = w - (L_u - k - a_u) (o = 1) the contig fits: 0 <= j and j + L_u <= L_v.  With KC_DEDUP_DUPLICATES_ONLY L_v == L_u
 * is required as well.
 * Mismatches of a candidate: the positions i in [0, L_u) at which (o ? rc(T_u) : T_u)[i] and T_v[j + i] differ as bytes; N
 * equals N.  A candidate is VERIFIED iff its mismatches <= max_mismatches.  u is REDUNDANT iff it has a verified candidate.
 * The record names one verified candidate: the one with the greatest v under the order above, then the smallest j, then the
 * smallest o.  status: KC_DEDUP_KEPT when u is not redundant, KC_DEDUP_DUPLICATE when the named v has L_v == L_u,
 * KC_DEDUP_CONTAINED otherwise.
 * Output block: the kept contigs in input order, each followed by '_'; depths_out is gathered the same way.  It is a block
 * that kc_ctg_index_build, kc_submit_ctg_block, kc_ctg_select and kc_fasta_text take as it is.
 *
 * Properties (tests/test_dedup_model.py holds the model to them).  With max_mismatches = 0 an anchored u is redundant exactly
 * when T_u or rc(T_u) is a substring of some T_v that outranks u, and the named container is itself kept.  With
 * max_mismatches > 0 the anchor must still match exactly -- a copy whose first all-ACGT window carries a difference is not
 * found -- and the named container may itself be redundant (containment within a distance is not transitive).
 *
 * kc_dedup_rec, one per input contig (recs may be NULL): status; container, pos = j, mismatches and orient = o of the named
 * candidate (container 0xFFFFFFFF, the others 0 when kept); new_index, the contig's index in the output block (0xFFFFFFFF
 * when removed); len = L_u; absorbed, the redundant contigs whose record names this one; flags KC_DEDUP_UNANCHORED.
 * Statistics: contigs, bases (the block without separators); anchored, unanchored; windows (of the whole block);
 * window_hits, the windows whose key is some contig's anchor key; candidates, verified; duplicates, contained, kept (contigs);
 * kept_bases, removed_bases, longest_removed.
 *
 * Protocol, kc_scaffold's.  Unknown flags, non-zero reserved words and NULL params / n_out / nbytes_out are KC_ERR_INVALID_ARG
 * in front of ctx, kc_last_error naming the value.  on_device applies to all arrays alike (params is the host's); device
 * records are 16-byte aligned, offsets 8-byte, depths 2-byte, seqs any.  seqs_out == NULL is a size query: *n_out (kept
 * contigs), *nbytes_out (their block's bytes) and *stats (may be NULL) are written and nothing else.  A capacity (bytes of
 * seqs_out; offsets_out has room for n_ctgs + 1 entries, depths_out for capacity) below *nbytes_out: KC_ERR_CAPACITY with the
 * same three written.  offsets_out and depths_out may be NULL; depths == NULL: depths_out is not written.  The block is
 * checked as kc_ctg_index_build checks it, with the same verdicts, before anything is stored.  More candidates than
 * max_candidates (0: 2^26) is KC_ERR_CAPACITY, kc_last_error naming both numbers, nothing written: the defined answer to
 * pathological repeats (n poly-A contigs give n x windows candidates), never a truncation.  n_ctgs == 0: KC_OK, an empty
 * block.  The call needs neither index, table nor results, works before or after kc_finalize and with rank_n > 1, runs on
 * the context's stream, returns when its work is done, keeps no state and frees its scratch: at most 84 bytes a
 * contig (the table included) and 8 for every word of its key, 16 bytes a candidate, 8 a kept contig, a byte for every 1024
 * of the block, beside the copies of host arrays.
 */
#define KC_DEDUP_DUPLICATES_ONLY 1u
#define KC_DEDUP_KEPT 0u
#define KC_DEDUP_DUPLICATE 1u
#define KC_DEDUP_CONTAINED 2u
#define KC_DEDUP_UNANCHORED 1u
typedef struct kc_dedup_params { /* 32 bytes */
  uint32_t max_mismatches;
  uint32_t flags;
  uint64_t max_candidates; /* 0: 2^26 */
  uint32_t reserved[4];    /* zero */
} kc_dedup_params;
typedef struct kc_dedup_rec { /* 32 bytes */
  uint32_t status;
  uint32_t container, pos, mismatches;
  uint32_t new_index, len, absorbed;
  uint8_t orient, flags;
  uint8_t reserved[2];
} kc_dedup_rec;
typedef struct kc_dedup_stats { /* 128 bytes */
  uint64_t contigs, bases;
  uint64_t anchored, unanchored;
  uint64_t windows, window_hits;
  uint64_t candidates, verified;
  uint64_t duplicates, contained;
  uint64_t kept, kept_bases, removed_bases, longest_removed;
  uint64_t reserved[2]; /* zero */
} kc_dedup_stats;
int kc_ctg_dedup(kc_ctx *ctx, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t n_ctgs, const uint16_t *depths,
                 int on_device, const kc_dedup_params *params, kc_dedup_rec *recs, uint8_t *seqs_out, uint64_t capacity,
                 uint64_t *offsets_out, uint16_t *depths_out, uint64_t *n_out, uint64_t *nbytes_out, kc_dedup_stats *stats);
/* ---- k-mer depths of sequences and the count spectrum (tests/kdepth_model.py) ------------------------
 * Two readers of the finished results.  The reference holds no code for either (it asks the table k-mer by k-mer,
 * KmerDHT::get_kmer_count, src/kcount/kmer_dht.cpp:198-245, and computes contig depths from such counts), so the rules below
 * are this project's own.
 *
 * kc_seq_kmer_depths: the depth track of sequences.  Sequence i is bytes [offsets[i], offsets[i+1]) of seqs; offsets[0] = 0,
 * offsets[nseqs] = nbytes, offsets never decrease, empty sequences are allowed.  One form serves reads (bases and offsets as
 * kc_align_reads takes them) and a seq block with its own offsets, where a contig's trailing '_' is simply its last byte.
 * A C G T a c g t are bases; every other byte (N, '_', anything) is not a base and is not an error.  With k the context's
 * kmer_len, position p of sequence i is a window iff p + k <= offsets[i+1] and all k bytes are bases; a window never spans two
 * sequences.  The window's key is the canonical k-mer of its upper-cased bytes, its count that k-mer's count among the results,
 * 0 when it is not there: purged as a singleton, below dmin_thres, with a fork or dead-end extension, or another rank's.
 *
 * track (nbytes values, may be NULL): track[p] is the window's count at a window start and 0 on every other byte.  With
 * KC_KDEPTH_FILL_MEAN track[p] is instead the sequence's mean on every base byte and 0 on every non-base byte: what
 * kc_submit_ctg_block takes, and what kc_build_unitigs writes as d_depths.  recs (one per sequence, may be NULL): sum of the
 * windows' counts; windows; present, those with a count above 0; solid, those with a count >= max(min_count, 1); min_count and
 * max_count over the present windows, 0 and 0 without one; mean = windows ? min(65535, (2 * sum + windows) / (2 * windows)) : 0.
 * stats (may be NULL): seqs, bytes, the totals of windows, present, solid and sum, and longest, the longest sequence in bytes.
 *
 * KC_ERR_STATE before kc_finalize.  rank_n > 1: own k-mers only; every k-mer lives on exactly one rank, so the ranks' tracks
 * (without KC_KDEPTH_FILL_MEAN), sums, present and solid add up to the single-rank answer.  The call uses the lookup index of
 * kc_lookup and builds it if absent; the results are not sorted, moved or touched, and earlier kc_result pointers stay valid.
 * KC_ERR_INVALID_ARG, before any device call: NULL ctx / params / offsets, NULL seqs with nbytes > 0, unknown flags, non-zero
 * reserved words, min_count > 65535, misaligned device arrays (offsets 8 bytes, track 2, recs 16); from the device check:
 * offsets that go backwards, offsets[0] != 0, offsets[nseqs] != nbytes.  KC_ERR_CAPACITY: a sequence of 2^32 bytes or more,
 * 2^32 sequences or more.  kc_last_error names the value.  On any error nothing is written.  nseqs == 0 or nbytes == 0: KC_OK
 * without a look at the offsets, zero stats, zero records, a zero track.  Positions are 64-bit, since a block of reads passes
 * 2^32 bytes; no test reaches that size.  The call runs on the context's stream and returns when its work there is done; its
 * scratch (32 bytes a sequence where records or means are asked for, the copies of host arrays) lives for the call.
 * on_device != 0: seqs, offsets, track and recs are device pointers.
 *
 * kc_count_spectrum: hist[c] (KC_SPECTRUM_BINS values) is the number of results whose count is c.  hist or stats may be NULL,
 * not both (KC_ERR_INVALID_ARG).  KC_ERR_STATE before kc_finalize.  With rank_n > 1 the ranks' histograms add.  on_device != 0:
 * hist is a device pointer (8-byte aligned); stats is always the host's.
 */
#define KC_KDEPTH_FILL_MEAN 1u
typedef struct kc_kdepth_params { /* 32 bytes */
  uint32_t min_count;             /* a window is "solid" when its count >= max(min_count, 1); at most 65535 */
  uint32_t flags;                 /* KC_KDEPTH_FILL_MEAN */
  uint32_t reserved[6];           /* zero */
} kc_kdepth_params;
typedef struct kc_kdepth_rec { /* 32 bytes, one per sequence */
  uint64_t sum;                /* sum of the windows' counts */
  uint32_t windows, present, solid;
  uint16_t min_count, max_count; /* over the present windows; 0 and 0 when there is none */
  uint16_t mean;                 /* windows ? min(65535, (2*sum + windows) / (2*windows)) : 0 */
  uint16_t reserved[3];          /* zero */
} kc_kdepth_rec;
typedef struct kc_kdepth_stats { /* 64 bytes */
  uint64_t seqs, bytes, windows, present, solid, sum, longest, reserved;
} kc_kdepth_stats;
int kc_seq_kmer_depths(kc_ctx *ctx, const uint8_t *seqs, uint64_t nbytes, const uint64_t *offsets, uint64_t nseqs, int on_device,
                       const kc_kdepth_params *params, uint16_t *track, kc_kdepth_rec *recs, kc_kdepth_stats *stats);
#define KC_SPECTRUM_BINS 65536
typedef struct kc_spectrum_stats { /* 64 bytes */
  uint64_t kmers, sum_counts;      /* = kc_stats.total_kmers, kc_stats.sum_counts */
  uint64_t max_count;              /* greatest count with a k-mer, 0 without results */
  uint64_t mode_count, mode_kmers; /* the count most k-mers have, the smallest on a tie; how many */
  uint64_t saturated;              /* hist[65535] */
  uint64_t reserved[2];
} kc_spectrum_stats;
int kc_count_spectrum(kc_ctx *ctx, uint64_t *hist, int on_device, kc_spectrum_stats *stats);
/* KmerDHT::kmer_exists / get_kmer_count / get_local_kmer_counts (src/kcount/kmer_dht.cpp:198-245) in bulk, against the
 * results kept in HBM: nq k-mers of num_longs words each, in either orientation; counts[i] = 0 (and left/right = 0)
 * when the k-mer did not survive.  The index over the results is built on the first call after kc_finalize.
 * left/right may be NULL.  on_device != 0: all pointers are device pointers. */
int kc_lookup(kc_ctx *ctx, const uint64_t *queries, uint64_t nq, int on_device, uint16_t *counts, uint8_t *left, uint8_t *right);
/* Every table entry before the purge, for tests of S5/S6: keys[n*num_longs], counts[n] (clipped to 65535),
 * exts[n*8] = left ACGT then right ACGT.  Call with NULLs to get n. */
int kc_dump_table(kc_ctx *ctx, uint64_t *keys, uint16_t *counts, uint16_t *exts, uint64_t *n);

int kc_get_stats(kc_ctx *ctx, kc_stats *out);

/* Geometry of the bucketed insert path; 0 in a field keeps the automatic choice.  Only for tests
 * (forcing the overflow paths with tiny capacities) and tuning runs; call right after
 * kc_create / kc_reset, before the first submit. */
typedef struct kc_tuning {
  uint32_t mode;          /* 0 auto (bucketed; compact records where k and the geometry allow), 1 global-table path only,
                             2 bucketed with wide records only */
  uint32_t writers;       /* level-1 writer workgroups (<= 512) */
  uint32_t p1, p2;        /* fan-out of level 1 / level 2: 1..1024 each */
  uint32_t slots;         /* LDS slots per region */
  uint32_t chunk1, chunk2;         /* records per chunk of the level-1 / level-2 chains: powers of two */
  uint32_t chain1_max, chain2_max; /* longest chain, in chunks, of a (writer,bucket) segment / a region */
  uint32_t arena1;        /* chunks in each writer's arena */
  uint64_t ovf_capacity;  /* records per overflow list */
} kc_tuning;
int kc_set_tuning(kc_ctx *ctx, const kc_tuning *t);

/* Per-kernel device time, measured with HIP events recorded on the stream the kernels are
 * launched on (role of the reference's GPUTimer / get_elapsed_time, gpu_common.hpp:83-105,
 * gpu_hash_table.hpp:172).  Needs KC_FLAG_TIME_KERNELS.  Fills up to max entries, *n = how many. */
typedef struct kc_kernel_time {
  char name[48];
  uint64_t launches;
  double total_ms;
} kc_kernel_time;
int kc_get_kernel_times(kc_ctx *ctx, kc_kernel_time *out, int max, int *n);
/* TB/s at which the level-1 arena this context chose took level 1's write pattern for a millisecond when it was
 * allocated (the better of two allocations is kept: which physical memory the driver hands out decides the rate, see
 * DESIGN.md section 5); 0 when no probe ran (arenas under a GiB, KC_ARENA_PROBE=0, the global-table path).  Lets a
 * caller see a slow draw; the library asks no absolute rate of an arena. */
int kc_arena_probe_rate(kc_ctx *ctx, double *tbps);
int kc_clear_kernel_times(kc_ctx *ctx);

/* ---- synthetic ArcticSynth-shaped reads (bench / tests) ------- */
typedef struct kc_synth_params {
  uint64_t seed;
  uint32_t num_genomes;    /* default 64 */
  uint32_t read_len;       /* default 150 */
  uint64_t min_genome_len; /* default 2,000,000 */
  uint64_t max_genome_len; /* default 6,000,000 */
  double sub_error_rate;   /* default 0.005 */
  double lowq_rate;        /* extra low-quality bases, default 0.01 */
  double n_rate;           /* default 0 */
  double abundance_sigma;  /* log-normal sigma, default 1.0 */
} kc_synth_params;

void kc_synth_default_params(kc_synth_params *p);
/* Reads [first_read, first_read+nreads) of the stream defined by p, written as
 * fixed-length records: bases/quals get nreads*read_len bytes, offsets nreads+1
 * entries (relative to this block).  The host and device versions produce the
 * same bytes. */
int kc_synth_reads_host(const kc_synth_params *p, uint64_t first_read, uint64_t nreads, uint8_t *bases, uint8_t *quals,
                        uint64_t *offsets);
int kc_synth_reads_device(kc_ctx *ctx, const kc_synth_params *p, uint64_t first_read, uint64_t nreads, uint8_t *d_bases,
                          uint8_t *d_quals, uint64_t *d_offsets);

#ifdef __cplusplus
}
#endif
#endif /* KCOUNT_MI355_H */
