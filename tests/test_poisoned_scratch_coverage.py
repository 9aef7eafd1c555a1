"""No entry point of the library arrives without a place in the poisoned-scratch tests ("Poisoned scratch"): every
extern "C" function of csrc/ is either COVERED -- named with the GPU test that runs it with KC_DEBUG_FILL set and compares
its results with a model -- or EXEMPT, with the reason in a line.  No GPU is needed here: the sources and the test modules
are read as text."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mhm2_kmer_analysis_v2_amd", "csrc")

CORE, FRONT, CTG = "test_gpu_poisoned_scratch_core", "test_gpu_poisoned_scratch_frontend", "test_gpu_poisoned_scratch_ctg"

# entry point -> (module, test); a wrapper of kcount.py that the test calls reaches the entry point
COVERED = {
    "kc_create": (CORE, "test_counting_core_equals_the_oracle"),
    "kc_destroy": (CORE, "test_counting_core_equals_the_oracle"),
    "kc_set_tuning": (CORE, "test_counting_core_equals_the_oracle"),
    "kc_submit_reads": (CORE, "test_counting_core_equals_the_oracle"),
    "kc_flush": (CORE, "test_counting_core_equals_the_oracle"),
    "kc_finalize": (CORE, "test_counting_core_equals_the_oracle"),
    "kc_copy_results": (CORE, "test_counting_core_equals_the_oracle"),
    "kc_dump_table": (CORE, "test_counting_core_equals_the_oracle"),
    "kc_get_stats": (CORE, "test_counting_core_equals_the_oracle"),
    "kc_reset": (CORE, "test_reset_to_another_width_and_back"),
    "kc_begin_ctg_kmers": (CORE, "test_contig_kmers_on_top_of_the_reads"),
    "kc_submit_ctg_block": (CORE, "test_contig_kmers_on_top_of_the_reads"),
    "kc_lookup": (CORE, "test_lookup_present_reverse_complement_and_absent"),
    "kc_submit_seq_block": (CORE, "test_other_input_forms_and_the_entries_copy"),
    "kc_submit_packed_reads": (CORE, "test_other_input_forms_and_the_entries_copy"),
    "kc_copy_results_entries": (CORE, "test_other_input_forms_and_the_entries_copy"),
    "kc_build_supermers": (CORE, "test_other_input_forms_and_the_entries_copy"),
    "kc_submit_packed_supermers": (CORE, "test_other_input_forms_and_the_entries_copy"),
    "kc_sort_results": (CORE, "test_sort_case_families_sort_and_dump"),
    "kc_dump_text_device": (CORE, "test_large_set_sorts_and_dumps"),
    "kc_build_unitigs": (CORE, "test_unitigs_equal_the_model"),
    "kc_fastq_to_packed_device": (FRONT, "test_fastq_parse"),
    "kc_fastq_pairs_device": (FRONT, "test_fastq_parse"),
    "kc_merge_pairs": (FRONT, "test_merge_pairs"),
    "kc_adapters_load": (FRONT, "test_trim_adapters"),
    "kc_adapters_clear": (FRONT, "test_trim_adapters"),  # (kc_adapters_load clears first)
    "kc_trim_adapters": (FRONT, "test_trim_adapters"),
    "kc_fastq_text": (FRONT, "test_fastq_text"),
    "kc_fasta_to_block": (FRONT, "test_fasta_to_block"),
    "kc_shard_extract": (FRONT, "test_single_pass_shard_flow"),
    "kc_shard_reserve": (FRONT, "test_single_pass_shard_flow"),
    "kc_shard_commit": (FRONT, "test_single_pass_shard_flow"),
    "kc_extract_partition": (FRONT, "test_records_flow"),
    "kc_insert_records": (FRONT, "test_records_flow"),
    "kc_wire_unit": (FRONT, "test_records_flow"),
    "kc_partition_owner": (FRONT, "test_records_flow"),
    "kc_extract_partition_seq_block": (FRONT, "test_seq_block_senders_and_record_pieces"),
    "kc_shard_extract_seq_block": (FRONT, "test_seq_block_senders_and_record_pieces"),
    "kc_insert_record_pieces": (FRONT, "test_seq_block_senders_and_record_pieces"),
    "kc_ctg_index_build": (CTG, "test_index_and_align_reads"),
    "kc_align_reads": (CTG, "test_index_and_align_reads"),
    "kc_align_gapped": (CTG, "test_align_gapped"),
    "kc_pair_inserts": (CTG, "test_pair_inserts_and_aln_depths"),
    "kc_aln_depths": (CTG, "test_pair_inserts_and_aln_depths"),
    "kc_local_assm": (CTG, "test_local_assm"),
    "kc_ctg_links": (CTG, "test_ctg_links_and_scaffolds"),
    "kc_scaffold": (CTG, "test_ctg_links_and_scaffolds"),
    "kc_close_gaps": (CTG, "test_close_gaps"),
    "kc_shuffle_reads": (CTG, "test_shuffle_reads"),
    "kc_ctg_select": (CTG, "test_selection_fasta_text_and_dedup"),
    "kc_fasta_text": (CTG, "test_selection_fasta_text_and_dedup"),
    "kc_ctg_dedup": (CTG, "test_selection_fasta_text_and_dedup"),
}

# what a wrapper named in a test goes through, where the name differs from the entry point's
WRAPPERS = {
    "kc_create": "KmerCounter(", "kc_destroy": "KmerCounter(", "kc_set_tuning": "tuning=", "kc_copy_results": "same_as_oracle(",
    "kc_get_stats": "same_as_oracle(", "kc_finalize": "same_as_oracle(", "kc_dump_table": "same_as_oracle(", "kc_submit_ctg_block": "submit_ctgs(", "kc_dump_text_device": "dump_text(",
    "kc_build_unitigs": "device_unitigs(", "kc_fastq_to_packed_device": "same_packed(", "kc_fastq_pairs_device": "same_pairs(",
    "kc_merge_pairs": "gpu_merge(", "kc_adapters_load": "load_adapters(", "kc_adapters_clear": "load_adapters(", "kc_trim_adapters": "gpu_trim(",
    "kc_fastq_text": "text_call(", "kc_fasta_to_block": "fasta_exact(", "kc_shard_extract": "run_shards(", "kc_shard_reserve": "run_shards(",
    "kc_shard_commit": "run_shards(", "kc_extract_partition": "run_flow(", "kc_insert_records": "run_flow(", "kc_wire_unit": "run_flow(",
    "kc_ctg_index_build": "Ctx(", "kc_insert_record_pieces": 'together="strided"', "kc_scaffold": ".scaffolds(", "kc_ctg_select": "select_contigs(", "kc_ctg_dedup": "dedup_contigs(",
}

EXEMPT = {
    "kc_abi_version": "allocates nothing: a constant",
    "kc_error_string": "allocates nothing: a table of strings",
    "kc_last_error": "allocates nothing: the thread's message",
    "kc_debug_filled_bytes": "allocates nothing: the counter the GPU tests read",
    "kc_device_count": "allocates nothing",
    "kc_num_longs": "allocates nothing: arithmetic on k",
    "kc_record_longs": "allocates nothing: arithmetic on k",
    "kc_owner": "allocates nothing: host arithmetic on one k-mer",
    "kc_owner_reference": "allocates nothing: host arithmetic on one k-mer",
    "kc_shard_owner": "allocates nothing: host arithmetic on one k-mer and the geometry",
    "kc_shard_capacity": "allocates nothing of its own: the geometry's arenas, which every counting test fills, and arithmetic",
    "kc_adapters_index": "host only: builds the adapter index in host memory and returns its counters",
    "kc_fastq_to_packed": "host only: the host parser, the reference of the device parser's test",
    "kc_fastq_pairs": "host only: the host parser, the reference of the device parser's test",
    "kc_synth_default_params": "host only: fills a struct",
    "kc_synth_reads_host": "host only: writes the caller's arrays",
    "kc_synth_reads_device": "its one allocation (the generator's table) is uploaded whole before the kernel reads it; pinned to the host "
                             "generator by test_device_and_host_generators_agree",
    "kc_set_stream": "allocates nothing: waits and stores a handle",
    "kc_ctg_stats": "allocates nothing: reads back two counters kc_begin_ctg_kmers zeroed",
    "kc_ctg_index_clear": "allocates nothing: frees the index",
    "kc_ctg_index_info": "allocates nothing: two host fields",
    "kc_get_kernel_times": "allocates nothing: host accumulators",
    "kc_clear_kernel_times": "allocates nothing: host accumulators",
    "kc_arena_probe_rate": "allocates nothing: a host field; the probe itself runs for arenas of a GiB and more only (DESIGN.md, open points)",
}


def entry_points():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".hpp")):
            src = open(os.path.join(CSRC, f)).read()
            names |= set(re.findall(r'extern "C"[^;{(]*?\b(kc_[a-z_0-9]+)\s*\(', src))
    return names


def test_every_entry_point_is_covered_or_exempt():
    names = entry_points()
    assert len(names) >= 70 and "kc_ctg_dedup" in names and "kc_create" in names
    assert not set(COVERED) & set(EXEMPT)
    missing = sorted(names - set(COVERED) - set(EXEMPT))
    assert not missing, "entry points without a poisoned-scratch test or a reason: %s" % missing
    stale = sorted((set(COVERED) | set(EXEMPT)) - names)
    assert not stale, "listed, but no entry point of csrc/: %s" % stale
    assert all(isinstance(r, str) and len(r) > 10 for r in EXEMPT.values())


def test_the_covering_tests_exist_set_the_fill_and_call_the_entry_point():
    body = {}
    for name, (module, test) in COVERED.items():
        if module not in body:
            src = open(os.path.join(ROOT, "tests", module + ".py")).read()
            assert "pytestmark = pytest.mark.gpu" in src and 'monkeypatch.setenv("KC_DEBUG_FILL"' in src and "kc_debug_filled_bytes()" in src, module
            body[module] = dict(re.findall(r"^def (test_\w+)\((.*?)(?=^def |^# ----|\Z)", src, flags=re.S | re.M))
        assert test in body[module], "%s: no test %s in %s" % (name, test, module)
        text = body[module][test]
        assert text.startswith("fill"), "%s::%s does not take the fill fixture" % (module, test)
        called = WRAPPERS.get(name, "." + name[3:] + "(")
        assert called in text or name in text, "%s::%s does not call %s (%s)" % (module, test, name, called)
