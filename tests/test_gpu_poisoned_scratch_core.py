"""No result of the counting core, the sort, the dump text or the unitigs depends on memory the library allocated and has
not written ("Poisoned scratch"): with KC_DEBUG_FILL set every fresh allocation of the library holds that byte,
and every case below still equals its oracle or model exactly.  Two fills a case: 0xA5 (as a signed word very negative, as an
unsigned one very large, neither 0 nor all ones: a missing zero, a missing 0xFF "none", a missing 0x7F minimum start show)
and 0x5A (large and positive: a missing 0x80 maximum start, which 0xA5 hides behind max).  Neither is a base, a digit, '_'
or a newline, so a stray byte in a text shows.  The contexts are made after the variable is set -- arenas and tables are
allocated at create and first use -- and every test checks that kc_debug_filled_bytes() rose across its device calls, so
that none passes because nothing was filled.  The expectations are the oracle's (computed once a case, cached here), numpy's
lexsort of the context's own unsorted results, and tests/unitig_model.py on the context's own results; none comes from the
code under test, only the device calls are repeated per fill.

Shapes: about 600 reads of a 900-base genome (a few hundred results, several level-1 writers and regions under the small
tunings); KC_HOST_BLOCK=8192 cuts their 40 KB into five blocks; the large sort set holds about 390 000 results -- 95 sort
tiles, 95 x 256 digit counters, three rounds of the 8192-item scan.  Wall time on the MI355X: 14 s for the module's 93
tests, the large sort set 1.2 s with its expectation, 0.3 s without."""
import numpy as np
import pytest

import mhm2_kmer_analysis_v2_amd as pkg
import sort_cases as S
import unitig_model as M
from helpers import random_reads
from oracle import cpu_oracle as O
from mhm2_kmer_analysis_v2_amd import _lib
from test_gpu_parity import PATHS, arrays, assert_same, oracle_run, pack_reads
from test_gpu_sort_dump import big_reads, model_text
from test_gpu_unitigs import arrays as hq_arrays
from test_gpu_unitigs import chain, circle_read, cover, device_unitigs, rand_seq
from test_gpu_wire import cut

pytestmark = pytest.mark.gpu

FILLS = (0xA5, 0x5A)
KS = (21, 33, 77)
# default, the global table, compact records, and test_overflow_paths_are_exact's "everything" (both chains overflow, the LDS
# tables fill, many chunks a chain)
TUNINGS = {
    "default": None,
    "table": PATHS["table"],
    "compact": PATHS["compact"],
    "overflow": dict(writers=4, p1=8, p2=8, slots=128, chunk1=16, chain1_max=6, chunk2=16, chain2_max=12, ovf_capacity=1 << 20),
}


@pytest.fixture(params=FILLS, ids=["0xA5", "0x5A"])
def fill(request, monkeypatch):
    monkeypatch.setenv("KC_DEBUG_FILL", "0x%02X" % request.param)
    before = pkg.lib().kc_debug_filled_bytes()
    yield request.param
    assert pkg.lib().kc_debug_filled_bytes() > before, "nothing was filled: the test proves nothing"


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def small_reads(seed, n=600):
    rng = np.random.default_rng(seed)
    return random_reads(rng, n, genome_len=900, err=0.01)


def small_case(k, seed=3):
    """(bases, quals, offsets), and the oracle's results, table and statistics for them"""
    def make():
        b, q, offs = arrays(*small_reads(seed))
        return (b, q, offs), oracle_run(b, q, offs, k)
    return cached(("small", k, seed), make)


def same_as_oracle(kc, want, wtable, wst):
    gtable = kc.dump_table()
    got = kc.sorted_results()
    st = kc.stats()
    assert_same(got, want)
    assert (gtable[0] == wtable[0]).all() and (gtable[1] == wtable[1]).all() and (gtable[2] == wtable[2]).all()
    assert st["raw_kmers"] == wst["raw_kmers"] and st["kmers_inserted"] == wst["kmers_inserted"]
    assert st["num_unique"] == wst["unique"] and st["num_purged"] == wst["purged"]
    assert st["total_kmers"] == wst["total_kmers"] and st["sum_counts"] == wst["sum_counts"] and st["num_dropped"] == 0


def test_nothing_is_filled_without_the_variable(monkeypatch):
    """unset and unparsable: today's behaviour, and the counter stands still"""
    (b, q, offs), (want, wtable, wst) = small_case(21)
    for value in (None, "", "256", "12x", "-1"):
        if value is None:
            monkeypatch.delenv("KC_DEBUG_FILL", raising=False)
        else:
            monkeypatch.setenv("KC_DEBUG_FILL", value)
        before = pkg.lib().kc_debug_filled_bytes()
        with pkg.KmerCounter(21) as kc:
            kc.submit_reads(b, q, offs)
            same_as_oracle(kc, want, wtable, wst)
        assert pkg.lib().kc_debug_filled_bytes() == before, value


# ---- the counting core ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(TUNINGS))
@pytest.mark.parametrize("k", KS)
def test_counting_core_equals_the_oracle(fill, k, path):
    (b, q, offs), (want, wtable, wst) = small_case(k)
    assert len(want[1]) > 100
    with pkg.KmerCounter(k, tuning=TUNINGS[path]) as kc:
        kc.submit_reads(b, q, offs)
        kc.flush()
        same_as_oracle(kc, want, wtable, wst)


@pytest.mark.parametrize("k", KS)
def test_host_input_in_several_blocks(fill, k, monkeypatch):
    monkeypatch.setenv("KC_HOST_BLOCK", "8192")
    (b, q, offs), (want, wtable, wst) = small_case(k)
    assert len(b) > 4 * 8192
    with pkg.KmerCounter(k) as kc:
        kc.submit_reads(b, q, offs)
        same_as_oracle(kc, want, wtable, wst)


def test_reset_to_another_width_and_back(fill):
    with pkg.KmerCounter(21) as kc:
        for k in (21, 77, 33, 21):
            (b, q, offs), (want, wtable, wst) = small_case(k)
            kc.reset(k)
            kc.submit_reads(b, q, offs)
            same_as_oracle(kc, want, wtable, wst)


def _short_and_n_reads(k):
    """small_case's reads with, among them, reads that give no k-mer: empty, shorter than k, of k and k + 1 bases (no k-mer
    with both neighbours), and all N"""
    reads, quals = small_reads(3)
    extra = ["", "ACGT", "A" * (k - 1), "ACGT" * k, "N" * (k + 40), ("ACGT" * k)[:k], ("ACGT" * k)[:k + 1]]
    for i, e in enumerate(extra):
        reads.insert(37 * i, e)
        quals.insert(37 * i, "I" * len(e))
    return reads, quals


@pytest.mark.parametrize("path", ["default", "table", "overflow"])
@pytest.mark.parametrize("k", KS)
def test_reads_that_give_no_kmer(fill, k, path):
    def make():
        b, q, offs = arrays(*_short_and_n_reads(k))
        return (b, q, offs), oracle_run(b, q, offs, k)
    (b, q, offs), (want, wtable, wst) = cached(("short", k), make)
    with pkg.KmerCounter(k, tuning=TUNINGS[path]) as kc:
        kc.submit_reads(b, q, offs)
        same_as_oracle(kc, want, wtable, wst)


@pytest.mark.parametrize("path", ["default", "table"])
@pytest.mark.parametrize("k", KS)
def test_no_reads_and_only_reads_without_kmers(fill, k, path):
    with pkg.KmerCounter(k, tuning=TUNINGS[path]) as kc:  # nothing submitted
        res = kc.sorted_results()
        assert len(res[1]) == 0 and res[0].shape == (0, kc.nl)
        assert kc.dump_text() == b"" and len(kc.dump_table()[1]) == 0
        st = kc.stats()
        assert st["raw_kmers"] == 0 and st["kmers_inserted"] == 0 and st["total_kmers"] == 0 and st["sum_counts"] == 0
        assert kc.lookup(np.zeros((3, kc.nl), dtype=np.uint64))[0].tolist() == [0, 0, 0]
        kc.reset()

        def make():
            b, q, offs = arrays(["", "ACGT", "A" * (k - 1), "N" * (k + 40), ("ACGT" * k)[:k + 1]], None)
            return (b, q, offs), oracle_run(b, q, offs, k)
        (b, q, offs), (want, wtable, wst) = cached(("nothing", k), make)
        assert len(want[1]) == 0 and wst["raw_kmers"] > 0
        kc.submit_reads(b, q, offs)
        kc.flush()
        same_as_oracle(kc, want, wtable, wst)
        assert kc.dump_text() == b""


@pytest.mark.parametrize("k", KS)
def test_contig_kmers_on_top_of_the_reads(fill, k):
    def make():
        rng = np.random.default_rng(900 + k)
        genome = "".join(rng.choice(list("ACGT"), size=900))
        reads, quals = [], []
        for _ in range(400):
            a = int(rng.integers(0, len(genome) - 160))
            ln = int(rng.integers(k + 2, 150))
            reads.append(genome[a:a + ln])
            quals.append("".join("I" if rng.random() > 0.03 else "#" for _ in range(ln)))
        ctgs, depths = [], []
        for i in range(12):
            a = int(rng.integers(0, len(genome) - 300))
            ctgs.append(genome[a:a + int(rng.integers(k + 2, 300))])
            depths.append(int(rng.integers(0, 40)))
        ctgs += [ctgs[0], ctgs[1][:k + 5] + "N" + ctgs[1][k + 6:], "ACGT"[:3], "".join(rng.choice(list("ACGT"), size=200))]  # a contig without a k-mer too
        depths += [depths[0] + 5, 7, 9, 13]
        b, q, offs = arrays(reads, quals)
        o = O.Oracle(k, nranks=3, nthreads=1)
        o.add_reads(b, q, offs)
        for c, d in zip(ctgs, depths):
            o.add_ctg(c, d)
        res = o.finalize()
        o.close()
        return (b, q, offs), ctgs, depths, res
    (b, q, offs), ctgs, depths, want = cached(("ctg", k), make)
    for tuning in (None, dict(mode=1)):
        with pkg.KmerCounter(k, tuning=tuning) as kc:
            kc.submit_reads(b, q, offs)
            kc.begin_ctg_kmers(sum(len(c) for c in ctgs))
            kc.submit_ctgs(ctgs[:5], depths[:5])
            kc.submit_ctgs(ctgs[5:], depths[5:])
            assert_same(kc.sorted_results(), want)
            st = kc.stats()
            assert st["total_kmers"] == len(want[1]) and st["sum_counts"] == int(want[1].astype(np.int64).sum())


@pytest.mark.parametrize("k", KS)
def test_lookup_present_reverse_complement_and_absent(fill, k):
    (b, q, offs), (want, wtable, _) = small_case(k)
    keys, counts, left, right = want
    def make():
        rng = np.random.default_rng(70 + k)
        kept = {tuple(int(x) for x in row) for row in keys}
        purged = np.stack([row for row in wtable[0] if tuple(int(x) for x in row) not in kept][:200])
        rnd = np.stack([O.pack_kmer("".join(rng.choice(list("ACGT"), size=k))) for _ in range(100)])
        rnd = np.stack([r for r in rnd if tuple(int(x) for x in r) not in kept and tuple(int(x) for x in O.revcomp(r, k)) not in kept])
        return np.stack([O.revcomp(keys[i], k) for i in range(0, len(keys), 3)]), purged, rnd
    rcq, purged, rnd = cached(("lookup", k), make)
    with pkg.KmerCounter(k) as kc:
        kc.submit_reads(b, q, offs)
        kc.flush()
        c, l, r = kc.lookup(keys)
        assert (c == counts).all() and (l == left).all() and (r == right).all()
        c2, l2, r2 = kc.lookup(rcq)
        assert (c2 == counts[::3]).all() and (l2 == left[::3]).all() and (r2 == right[::3]).all()
        for absent in (purged, rnd):
            c3, l3, r3 = kc.lookup(absent)
            assert (c3 == 0).all()
        assert len(kc.lookup(np.zeros((0, kc.nl), dtype=np.uint64))[0]) == 0
        kc.sort_results()  # the index is built again over the new order
        c4, l4, r4 = kc.lookup(keys[::5])
        assert (c4 == counts[::5]).all() and (l4 == left[::5]).all() and (r4 == right[::5]).all()


@pytest.mark.parametrize("k", KS)
def test_other_input_forms_and_the_entries_copy(fill, k):
    """the same reads as a '_'-joined block of case-masked reads, as the read cache's packed bytes (host and device, the device
    array at an odd address), and as supermers cut, packed and unpacked again; kc_copy_results_entries on the sorted results"""
    import torch
    reads, quals = small_reads(3)
    (b, q, offs), (want, wtable, wst) = small_case(k)
    masked = cached(("masked", k), lambda: ["".join(c.lower() if ord(x) < 33 + 20 else c for c, x in zip(r, ql)) for r, ql in zip(reads, quals)])
    packed = cached(("packed", k), lambda: pack_reads(reads, quals))
    block = ("_".join(masked) + "_").encode()
    with pkg.KmerCounter(k) as kc:
        kc.submit_seq_block(block)
        assert_same(kc.sorted_results(), want)
        assert kc.stats()["raw_kmers"] == wst["raw_kmers"]
        kc.reset()
        kc.submit_packed_reads(packed, offs)
        same_as_oracle(kc, want, wtable, wst)
        kc.reset()
        dp = torch.zeros(len(packed) + 32, dtype=torch.uint8, device="cuda")
        dp[5:5 + len(packed)] = torch.from_numpy(packed).cuda()
        kc.submit_packed_reads(dp[5:], torch.from_numpy(offs.astype(np.int64)).cuda(), nreads=len(reads))
        assert_same(kc.sorted_results(), want)
        n = int(kc.sort_results().n)
        keys = np.zeros((n, kc.nl), dtype=np.uint64)
        vals = np.zeros(n, dtype=np.dtype([("count", np.uint32), ("left", np.int8), ("right", np.int8), ("pad", np.int8, 2)]))
        _lib.check(pkg.lib().kc_copy_results_entries(kc._h, keys.ctypes.data, vals.ctypes.data), "kc_copy_results_entries")
        assert (keys == want[0]).all() and (vals["count"] == want[1]).all()
        assert (vals["left"].astype(np.uint8) == want[2]).all() and (vals["right"].astype(np.uint8) == want[3]).all()
    nranks = 2

    def supermers():
        o = O.Oracle(k, nranks=nranks, nthreads=2)
        starts = np.cumsum([0] + [len(m) + 1 for m in masked])
        out = {(t, int(s0) + st, ln) for m, s0 in zip(masked, starts) for t, st, ln in o.supermers(m)}
        o.close()
        return out
    want_sm = cached(("supermers", k), supermers)
    with pkg.KmerCounter(k, rank_me=0, rank_n=nranks) as kc:
        targets, offsets, lens, nvalid, pk = kc.build_supermers(block)
    got = set(zip(targets.tolist(), offsets.tolist(), lens.tolist()))
    assert got == want_sm and len(got) == len(targets) and nvalid == wst["kmers_inserted"]
    per_target = [bytearray() for _ in range(nranks)]
    for t, off, ln in sorted(got):
        per_target[t] += cut(pk, off, ln) + b"_"
    parts = []
    for t in range(nranks):
        with pkg.KmerCounter(k) as kc:
            if per_target[t]:
                kc.submit_packed_supermers(np.frombuffer(bytes(per_target[t]), dtype=np.uint8))
            parts.append(kc.results())
    assert_same(lexsorted(tuple(np.concatenate([p[i] for p in parts]) for i in range(4))), want)


# ---- sort and dump ---------------------------------------------------------------------------------------------------------
def lexsorted(res):
    keys, counts, left, right = res
    order = np.lexsort([keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)]) if len(counts) else np.zeros(0, dtype=np.int64)
    return keys[order], counts[order], left[order], right[order]


@pytest.mark.parametrize("k", [21, 33])
def test_sort_case_families_sort_and_dump(fill, k):
    """every family of tests/sort_cases.py, "empty" and "one k-mer" among them, on one context: a smaller set follows a
    larger one in the kept blocks"""
    fams = cached(("families", k), lambda: [(f.name, f.arrays(), f.expected()) for f in S.families(k)])
    assert {"empty", "one k-mer"} <= {name for name, _, _ in fams}
    with pkg.KmerCounter(k) as kc:
        for name, (b, q, offs), want in fams:
            kc.reset()
            kc.submit_reads(b, q, offs)
            unsorted = kc.results()
            assert_same(lexsorted(unsorted), want)
            r = kc.sort_results()
            assert int(r.n) == len(want[1]), name
            assert_same(kc.results(), want)
            text = cached(("family text", k, name), lambda: model_text(want, k))
            assert kc.dump_text() == text, name
            n = len(want[1])
            if n > 10:  # a window whose first line is no multiple of the 256 lines a tile
                part = cached(("family part", k, name), lambda: model_text(tuple(a[7:n - 3] for a in want), k))
                assert kc.dump_text(7, n - 10, sort=False) == part, name


def test_large_set_sorts_and_dumps(fill):
    """more than 131 072 results: the 256-counters-a-tile array passes 8192 and the scan carries"""
    k = 21
    with pkg.KmerCounter(k) as kc:
        kc.submit_reads(*big_reads())
        unsorted = kc.results()
        assert len(unsorted[1]) > 131072

        def make():
            want = lexsorted(unsorted)
            first, count = 1001, 5 * 256 + 77
            return want, model_text(want, k), (first, count, model_text(tuple(a[first:first + count] for a in want), k))
        want, text, (first, count, part) = cached("big", make)
        assert_same(lexsorted(unsorted), want)  # the same set under either fill: the text was made from it once
        r = kc.sort_results()
        assert int(r.n) == len(want[1])
        assert_same(kc.results(), want)
        got = kc.dump_text()
        assert len(got) == len(text) and got == text
        assert kc.dump_text(first, count, sort=False) == part


# ---- unitigs ---------------------------------------------------------------------------------------------------------------
def unitig_cases(k):
    rng = np.random.default_rng(5100 + k)
    s = rand_seq(rng, 90)
    cases = {
        "chains of 1, 2 and 65": sum((cover(chain(rng, m, k), k, times=2 + i % 2) for i, m in enumerate((1, 2, 65))), []),
        "a circle of 3": [circle_read("ACG", k)] * 2,
        "hairpin": [s + M.revcomp(s)] * 3,
        "no results": [rand_seq(rng, 100)],  # every k-mer once: all purged
    }
    return cases


@pytest.mark.parametrize("k", [21, 33])
def test_unitigs_equal_the_model(fill, k):
    cases = cached(("unitig cases", k), lambda: unitig_cases(k))
    for name, reads in cases.items():
        with pkg.KmerCounter(k) as kc:
            kc.submit_reads(*hq_arrays(reads))
            res = kc.results()

            def make():
                R = M.results_dict(*res, kc.k) if len(res[1]) else {}  # (the model's reshape takes no empty set)
                units, st = M.unitigs(R, kc.k)
                return lexsorted(res), units, st, M.block(units)
            want_res, units, st, (seqs, depths, offsets, sums) = cached(("unitigs", k, name), make)
            assert_same(lexsorted(res), want_res)  # the same results under either fill: the model ran on them once
            g_seqs, g_depths, g_offsets, g_sums, g_st = device_unitigs(kc)
            assert g_st == st, name
            assert g_seqs == seqs and (g_offsets == offsets).all() and (g_sums == sums).all() and (g_depths == depths).all(), name
            if name == "no results":
                assert g_seqs == b"" and g_offsets.tolist() == [0] and st["unitigs"] == 0
            else:
                assert st["unitigs"] >= 1
            if name == "a circle of 3":
                assert st["circular"] == 1
            # the wrapper's own arrays (kcount._Out) are filled too: the same block through it
            blk = kc.unitigs()
            assert bytes(blk[0].cpu().numpy().tobytes()) == seqs and (blk[1].cpu().numpy().astype(np.uint64) == offsets).all(), name


def test_palindromic_kmer_at_even_k(fill):
    k = 22
    def reads():
        rng = np.random.default_rng(5500 + k)
        h = rand_seq(rng, k // 2)
        return h + M.revcomp(h), [rand_seq(rng, 60) + h + M.revcomp(h) + rand_seq(rng, 60)] * 2
    p, rd = cached("palindrome reads", reads)
    with pkg.KmerCounter(k) as kc:
        kc.submit_reads(*hq_arrays(rd))
        res = kc.results()

        def make():
            R = M.results_dict(*res, kc.k)
            units, st = M.unitigs(R, kc.k)
            return lexsorted(res), R, units, st, M.block(units)
        want_res, R, units, st, (seqs, depths, offsets, sums) = cached("palindrome", make)
        assert_same(lexsorted(res), want_res)
        assert p in R and (p, R[p][0], R[p][0], 1) in units and st["unitigs"] == 3 and st["singletons"] == 1
        g_seqs, g_depths, g_offsets, g_sums, g_st = device_unitigs(kc)
        assert g_st == st and g_seqs == seqs and (g_offsets == offsets).all() and (g_sums == sums).all() and (g_depths == depths).all()
