// Exercises kcount_driver.hpp the way src/kcount/kcount_gpu.cpp drives the reference's device drivers:
// sender bins a '_'-joined block by target, receivers take records (or supermers), done_all_inserts,
// iterate.  Prints "KMER count L R" lines (kmer_dht.cpp:284 format), sorted, for the Python test to compare.
//
//   test_driver K MODE [ranks=R] [count=C] [repeat=N] [mem=BYTES] [cuts=a,b,...] [ctg_elems=N]
//
// stdin, one item per line:   a case-masked read;   ">depth sequence" a contig;   "=count sequence" a supermer that goes
// to insert_supermer with a count of its own (mode packed).
//   ranks      target ranks of the modes with a sender (records, wire, wirectg); default 2
//   count      the count every read's supermer is handed over with in mode packed; default 1
//   repeat     how often every read is handed to insert_supermer_ascii in mode ascii; default 1
//   mem        init's gpu_avail_mem; default 0 (unknown: the buffer is sized from max_elems alone)
//   cuts       line numbers at which the sender's block ends: the lines up to the first cut are block 0 and so on, what
//              is left is the last block.  The lines of a block are joined by '_' with none behind the last, so that a
//              block can have any length; without cuts everything is one block with a '_' behind every read
//   ctg_elems  init_ctg_kmers' max_elems; default 100000
// MAX_K follows k as the reference's build does: kc_num_longs(k) words, 32 / 64 / 96 / 128.
// What the tests read besides the dump goes to stderr, one "INFO ..." line each.  Exit codes: 2 the sender refused the
// block, 3 dropped, 4 target out of range, 5 k-mers not covered once, 6 sender timers, 7 receiver timers, 8 pass_type,
// 9 contig-pass attempts, 10 mode move flushed early, 11 attempted, 12 capacities, 13 kernel time, 14 bad arguments.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../mhm2_kmer_analysis_v2_amd/csrc/kcount_driver.hpp"

using namespace kcount_mi355;

template <int MAX_K>
static std::string kmer_str(const KmerArray<MAX_K> &k, int len) {
  std::string s;
  for (int i = 0; i < len; i++) s.push_back("ACGT"[(k.longs[i / 32] >> (2 * (31 - (i % 32)))) & 3]);
  return s;
}

static std::string pack(const std::string &read) {  // 4-bit packed as parse_and_pack.cpp:196-237 packs it
  static const std::string codes = "_acgtACGTN";
  std::string packed((read.size() + 1) / 2, '\0');
  for (size_t i = 0; i < read.size(); i++) {
    unsigned v = read[i] == 'n' ? 9u : (unsigned)codes.find(read[i]);  // N and n share code 9
    packed[i / 2] |= (char)(i % 2 ? v : v << 4);
  }
  return packed;
}

struct Options {
  int ranks = 2;
  count_t count = 1;
  int repeat = 1;
  size_t mem = 0;
  std::vector<size_t> cuts;
  uint64_t ctg_elems = 100000;
};

struct Input {
  std::vector<std::string> reads;
  std::vector<std::pair<count_t, std::string>> ctgs;      // ">depth sequence"
  std::vector<std::pair<count_t, std::string>> counted;   // "=count sequence"
};

static int reference_minimizer_len(int k) {  // kmer_dht.cpp:117-119
  int m = k * 2 / 3 + 1;
  m = m < 15 ? 15 : m > 27 ? 27 : m;
  return m < k ? m : k;
}

// The reference's own flow, step for step as its host file drives the two drivers (process_block,
// src/kcount/kcount_gpu.cpp:110-165): supermers and the packed block from the sender driver, every supermer's bytes
// cut out of the packed block with the odd nibbles masked, handed to the driver of its target rank.  depth_block: empty
// for reads (count 1), else the depth of every character's contig (the count is that of the character at offset + 1).
// -1: the sender refused the block.
template <int MAX_K>
static int send_wire(ParseAndPackDriver &pnp, const std::string &block, const std::vector<count_t> &depth_block,
                     std::vector<std::unique_ptr<HashTableDriver<MAX_K>>> &ht, int k, int index, uint64_t &sent) {
  const int R = (int)ht.size();
  unsigned nvalid = 0;
  const bool ok = pnp.process_seq_block(block, nvalid);
  if (ok) pnp.pack_seq_block(block);
  std::cerr << "INFO block " << index << " len=" << block.size() << " ok=" << ok << " supermers=" << pnp.supermers.size()
            << " valid=" << nvalid << " packed=" << pnp.packed_seqs.size() << "\n";
  if (!ok) return -1;
  uint64_t covered = 0;
  for (size_t i = 0; i < pnp.supermers.size(); i++) {
    const int target = pnp.supermers[i].target, offset = pnp.supermers[i].offset, len = pnp.supermers[i].len;
    int packed_len = len / 2;
    if (offset % 2 || len % 2) packed_len++;
    std::string seq = pnp.packed_seqs.substr(offset / 2, packed_len);
    if (offset % 2) seq[0] &= 15;
    if ((offset + len) % 2) seq[seq.length() - 1] &= (char)240;
    if (target < 0 || target >= R) return 4;
    ht[target]->insert_supermer(seq, depth_block.empty() ? (count_t)1 : depth_block[offset + 1]);
    covered += len - k - 1;
    sent++;
  }
  if (covered != nvalid) return 5;  // every k-mer with two neighbours is in exactly one supermer
  return 0;
}

template <int MAX_K>
static int run(int k, const std::string &mode, const Options &opt, const Input &in) {
  using Driver = HashTableDriver<MAX_K>;
  std::vector<std::string> blocks;
  if (opt.cuts.empty()) {
    std::string block;
    for (auto &r : in.reads) block += r + "_";
    blocks.push_back(block);
  } else {
    size_t at = 0;
    for (size_t c = 0; c <= opt.cuts.size(); c++) {
      const size_t end = c < opt.cuts.size() ? opt.cuts[c] : in.reads.size();
      if (end < at || end > in.reads.size()) return 14;
      std::string block;
      for (size_t i = at; i < end; i++) block += (i > at ? "_" : "") + in.reads[i];
      if (c < opt.cuts.size() || end > at) blocks.push_back(block);
      at = end;
    }
  }
  const bool strict = opt.cuts.empty();  // a refused block ends the run (exit code 2) unless the test cut the blocks itself
  const bool one_shard = mode == "ascii" || mode == "packed" || mode == "ctg" || mode == "move";
  const int R = one_shard ? 1 : opt.ranks;
  std::vector<std::string> out;
  std::string msgs, warnings;
  double t = 0;
  std::vector<std::unique_ptr<Driver>> ht;
  for (int r = 0; r < R; r++) {
    ht.emplace_back(new Driver());
    ht[r]->init(r, R, k, 100000, 0, 10000, opt.mem, msgs, warnings, false);
  }
  std::cerr << "INFO msgs " << msgs;
  if (!warnings.empty()) std::cerr << "INFO warnings " << warnings;
  uint64_t expect_attempted = 0;  // of shard 0, where a mode knows it
  if (mode == "records") {
    ParseAndPackDriver pnp(0, R, 33, k, kc_num_longs(k), 15, t, /*records_mode=*/true);
    for (size_t b = 0; b < blocks.size(); b++) {
      unsigned nvalid = 0;
      const bool ok = pnp.process_seq_block(blocks[b], nvalid);
      std::cerr << "INFO block " << b << " len=" << blocks[b].size() << " ok=" << ok << " valid=" << nvalid
                << " segment=" << pnp.segment_capacity() << "\n";
      if (!ok) {
        if (strict) return 2;
        continue;
      }
      for (int r = 0; r < R; r++)
        ht[r]->insert_records(pnp.records() + (size_t)r * pnp.segment_capacity() * pnp.record_longs(), pnp.counts()[r]);
    }
  } else if (mode == "wire" || mode == "wirectg") {
    ParseAndPackDriver pnp(0, R, 33, k, kc_num_longs(k), reference_minimizer_len(k), t);
    uint64_t sent = 0;
    for (size_t b = 0; b < blocks.size(); b++) {
      const int rc = send_wire<MAX_K>(pnp, blocks[b], {}, ht, k, (int)b, sent);
      if (rc > 0 || (rc < 0 && strict)) return rc < 0 ? 2 : rc;
    }
    if (mode == "wirectg") {
      // the second pass of a multi-round MHM2 run in the reference's own call order (kcount.cpp:106-139,
      // kmer_dht.cpp:158-171, kcount_gpu.cpp:167-180): every table is told that contig k-mers follow, the contigs go
      // through the sender as one '_'-joined block with the depth of every character beside it
      for (auto &h : ht) {
        h->flush_inserts();
        h->init_ctg_kmers(opt.ctg_elems, 0);
        if (h->pass_type != CTG_KMERS_PASS) return 8;
      }
      std::string block;
      std::vector<count_t> depth_block;
      for (auto &c : in.ctgs) {
        block += c.second + "_";
        depth_block.insert(depth_block.end(), c.second.size() + 1, c.first);
      }
      sent = 0;
      const int rc = send_wire<MAX_K>(pnp, block, depth_block, ht, k, (int)blocks.size(), sent);
      if (rc) return rc < 0 ? 2 : rc;
      uint64_t attempted_sum = 0;
      for (auto &h : ht) {
        h->flush_inserts();
        uint64_t attempted = 0, dropped = 0, fresh = 0;
        h->done_ctg_kmer_inserts(attempted, dropped, fresh);
        if (dropped) return 9;
        attempted_sum += attempted;
      }
      std::cerr << "INFO ctg supermers sent=" << sent << " attempted=" << attempted_sum << "\n";
      if (attempted_sum != sent) return 9;
    }
    auto [tf, tk] = pnp.get_elapsed_times();
    if (!(tf > 0 && tk > 0 && tf >= tk)) return 6;
  } else if (mode == "move") {
    // kcount_gpu.cpp:218-219 builds the state's member from a temporary; here the driver moves after init, with
    // supermers buffered and not yet flushed, and the moved-from one is destroyed before the rest goes in
    const size_t half = in.reads.size() / 2;
    for (size_t i = 0; i < half; i++) ht[0]->insert_supermer(pack(in.reads[i]), 1);
    if (ht[0]->get_num_gpu_calls() != 0) return 10;  // (nothing may have been flushed yet: that is the case this mode is for)
    std::unique_ptr<Driver> moved(new Driver(std::move(*ht[0])));
    ht[0].reset();
    ht[0] = std::move(moved);
    for (size_t i = half; i < in.reads.size(); i++) ht[0]->insert_supermer(pack(in.reads[i]), 1);
    expect_attempted = in.reads.size();
  } else {
    // whole reads as supermers into one shard
    for (auto &read : in.reads) {
      if (mode == "ascii") {
        for (int i = 0; i < opt.repeat; i++) ht[0]->insert_supermer_ascii(read);
        expect_attempted += opt.repeat;
      } else {
        ht[0]->insert_supermer(pack(read), opt.count);
        expect_attempted++;
      }
    }
    for (auto &s : in.counted) ht[0]->insert_supermer(pack(s.second), s.first);
    expect_attempted += in.counted.size();
    if (mode == "ctg") {
      // the second pass of a multi-round MHM2 run (kcount.cpp:106-139, kmer_dht.cpp:158-171): the table is told that
      // contig k-mers follow, every contig arrives as a supermer whose count is the contig's depth
      ht[0]->flush_inserts();
      ht[0]->init_ctg_kmers(opt.ctg_elems, 0);
      if (ht[0]->pass_type != CTG_KMERS_PASS) return 8;
      for (auto &c : in.ctgs) ht[0]->insert_supermer(pack(c.second), c.first);
      ht[0]->flush_inserts();
      uint64_t attempted = 0, dropped = 0, fresh = 0;
      ht[0]->done_ctg_kmer_inserts(attempted, dropped, fresh);
      if (attempted != in.ctgs.size() || dropped) return 9;
      std::cerr << "ctg: " << attempted << " supermers, " << fresh << " new k-mers\n";
    }
  }
  for (int r = 0; r < R; r++) {
    ht[r]->flush_inserts();
    uint64_t dropped, unique, purged;
    ht[r]->done_all_inserts(dropped, unique, purged);
    if (dropped) return 3;
    double t_ins = 0, t_ker = 0;
    ht[r]->get_elapsed_time(t_ins, t_ker);
    if (!(t_ins > 0 && t_ker > 0)) return 7;  // the timers are filled (gpu_hash_table.hpp:172)
    ht[r]->begin_iterate();
    uint64_t entries = 0;
    while (true) {
      auto [key, val] = ht[r]->get_next_entry();
      if (!key) break;
      entries++;
      out.push_back(kmer_str<MAX_K>(*key, k) + " " + std::to_string(val->count) + " " + (char)val->left + " " + (char)val->right);
    }
    std::cerr << "INFO rank " << r << " calls=" << ht[r]->get_num_gpu_calls() << " attempted=" << ht[r]->get_stats().attempted
              << " entries=" << entries << " capacity=" << ht[r]->get_capacity() << "\n";
    // the kernel time is that of every kind the context launched: all entries of kc_get_kernel_times, asked for by their
    // number first
    int n = 0;
    check(kc_get_kernel_times(ht[r]->handle(), nullptr, 0, &n), "kc_get_kernel_times");
    std::vector<kc_kernel_time> kt(n > 0 ? n : 1);
    check(kc_get_kernel_times(ht[r]->handle(), kt.data(), n, &n), "kc_get_kernel_times");
    double sum = 0;
    for (int i = 0; i < n; i++) sum += kt[i].total_ms * 1e-3;
    char line[160];
    std::snprintf(line, sizeof(line), "INFO kernel rank=%d kinds=%d driver=%.9e all=%.9e\n", r, n, t_ker, sum);
    std::cerr << line;
    if (!(std::fabs(t_ker - sum) <= 1e-9 * sum)) return 13;  // (only the order of a floating-point sum may differ)
    if (one_shard && ht[r]->get_stats().attempted != expect_attempted) return 11;
    if (!(ht[r]->get_capacity() > 0) || (uint64_t)ht[r]->get_final_capacity() != entries) return 12;
    ht[r].reset();
  }
  std::sort(out.begin(), out.end());
  for (auto &l : out) std::cout << l << "\n";
  return 0;
}

int main(int argc, char **argv) {
  const int k = argc > 1 ? atoi(argv[1]) : 21;
  const std::string mode = argc > 2 ? argv[2] : "records";
  Options opt;
  for (int i = 3; i < argc; i++) {
    const std::string a = argv[i];
    const size_t eq = a.find('=');
    if (eq == std::string::npos) return 14;
    const std::string key = a.substr(0, eq), val = a.substr(eq + 1);
    if (key == "ranks") opt.ranks = atoi(val.c_str());
    else if (key == "count") opt.count = (count_t)strtoull(val.c_str(), nullptr, 10);
    else if (key == "repeat") opt.repeat = atoi(val.c_str());
    else if (key == "mem") opt.mem = (size_t)strtoull(val.c_str(), nullptr, 10);
    else if (key == "ctg_elems") opt.ctg_elems = strtoull(val.c_str(), nullptr, 10);
    else if (key == "cuts") {
      for (size_t p = 0; p < val.size();) {
        size_t e = val.find(',', p);
        if (e == std::string::npos) e = val.size();
        opt.cuts.push_back((size_t)strtoull(val.substr(p, e - p).c_str(), nullptr, 10));
        p = e + 1;
      }
    } else return 14;
  }
  if (opt.ranks < 1 || opt.repeat < 1) return 14;
  Input in;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (!line.empty() && (line[0] == '>' || line[0] == '=')) {
      const size_t sp = line.find(' ');
      if (sp == std::string::npos) return 14;
      auto &list = line[0] == '>' ? in.ctgs : in.counted;
      list.emplace_back((count_t)strtoull(line.c_str() + 1, nullptr, 10), line.substr(sp + 1));
    } else {
      in.reads.push_back(line);
    }
  }
  switch (kc_num_longs(k)) {  // MAX_K as the reference's build picks it for this k
    case 1: return run<32>(k, mode, opt, in);
    case 2: return run<64>(k, mode, opt, in);
    case 3: return run<96>(k, mode, opt, in);
    case 4: return run<128>(k, mode, opt, in);
  }
  return 14;
}
