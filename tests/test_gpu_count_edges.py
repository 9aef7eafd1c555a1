"""The count / vote path (kc_count_kernel, vote_ext, kc_finalize_kernel, the flagged-region and merge-into-table paths) on
inputs whose answer is known by construction (tests/count_cases.py): the vote at its thresholds, the 16-bit counters at
65535, sums across buffer passes.  Everything is exact and is compared with the oracle AND with the expectation of every
case; every test proves from kernel_times() which path it took.  Need a real MI355X."""
import numpy as np
import pytest

import count_cases as CC
import mhm2_kmer_analysis_v2_amd as pkg
from oracle import cpu_oracle as O
from test_gpu_parity import l2_launches

pytestmark = pytest.mark.gpu

FLAGGED = "kc_flagged_to_table_kernel"
EXTRACT_INSERT = "kc_extract_kernel<insert>"
MERGE = "kc_insert_records_kernel"  # (kc_merge_entries_kernel is timed under this name)

# the count paths: k and the tuning that selects the instantiation
PATHS = {
    "default": (21, dict()),
    "compact": (21, dict(p1=256, p2=256)),             # 32-bit keys, EW = 6
    "compact-short": (21, dict(p1=1024, p2=512)),      # ... behind six-byte level-1 records
    "wide": (21, dict(mode=2, p1=256, p2=256)),        # one-word keys, EW = 6
    "two-word-33": (33, dict()),
    "two-word-51": (51, dict()),
    "n-word-77": (77, dict()),
    "n-word-125": (125, dict()),
    "table": (21, dict(mode=1)),                       # the global table: no regions
}
BUCKETED = [p for p in PATHS if p != "table"]
# a region of 65535 records stays in its chain (64 chunks of 1024) instead of overflowing to the list, which the LDS
# kernel never sees; the level-1 chains of the one bucket all those records share are long enough too
LONG_CHAINS = dict(chunk2=1024, chain2_max=72, chain1_max=160)
# ... and where the buffer is small, and a writer's share of a bucket large, in chunks of 1024 records
SMALL_BUFFER = dict(LONG_CHAINS, chunk1=1024)

_oracle = {}


def oracle_of(family, k, dmin_thres, cases, blocks):
    """(results, table, stats, entry by key, result by key) of the oracle: once per (family, k, dmin_thres)"""
    key = (family, k, dmin_thres)
    if key not in _oracle:
        o = O.Oracle(k, dmin_thres=dmin_thres, nranks=3, nthreads=2)
        for b, q, offs in blocks:
            o.add_reads(b, q, offs)
        table = o.dump_table()
        res = o.finalize()
        st = o.stats()
        o.close()
        assert st["dropped"] == 0
        entry = {tuple(int(x) for x in table[0][i]): (int(table[1][i]), [int(x) for x in table[2][i]]) for i in range(len(table[1]))}
        result = {tuple(int(x) for x in res[0][i]): (int(res[1][i]), chr(res[2][i]), chr(res[3][i])) for i in range(len(res[1]))}
        _oracle[key] = (res, table, st, entry, result)
    return _oracle[key]


_families = {}


def family(name, k, dmin_thres=2, n=None):
    """the cases of a family and their blocks of reads, built once"""
    key = (name, k, dmin_thres, n)
    if key not in _families:
        cases = {"grid": lambda: CC.vote_grid(k, dmin_thres), "fill": lambda: CC.region_fill(k, n),
                 "two-pass": lambda: CC.two_pass(k)}[name]()
        nblocks = max(len(c.blocks) for c in cases)
        _families[key] = (cases, [CC.emit(cases, k, 1000 + 10 * b, block=b) for b in range(nblocks)])
    return _families[key]


_saturation = {}


def saturation_cases(k, n):
    """[(case, its reads)] of the four flank splits of n occurrences: every case is a submission of its own"""
    if (k, n) not in _saturation:
        _saturation[k, n] = [(c, CC.emit([c], k, 2000 + c.tags["split"])) for c in CC.saturation(k) if c.tags["n"] == n]
    return _saturation[k, n]


def same(got, want, what):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, ("keys", "counts", "third", "fourth")):
        assert g.shape == w.shape, "%s %s: %s vs %s" % (what, name, g.shape, w.shape)
        if not (g == w).all():
            i = int(np.argwhere(np.asarray(g != w).reshape(len(g), -1).any(axis=1))[0][0])
            raise AssertionError("%s %s differ first at sorted entry %d: got %s want %s" % (what, name, i, g[i], w[i]))


def check_stats(st, cases, dmin_thres, ost, raw=True):
    """stats() against the construction and against the oracle's; raw=False for the records and shard flows: raw_kmers
    is counted where submit_reads extracts, and their extraction kernels do not report it"""
    est = CC.expected_stats(cases, dmin_thres)
    got = {f: st[f] for f in est}
    assert got == est
    assert st["num_dropped"] == 0
    assert (st["num_unique"], st["num_purged"], st["total_kmers"], st["sum_counts"], st["kmers_inserted"]) == (
        ost["unique"], ost["purged"], ost["total_kmers"], ost["sum_counts"], ost["kmers_inserted"])
    if raw:
        assert st["raw_kmers"] == ost["raw_kmers"]


def read_out(kc):
    """(pre-purge table, sorted results, stats, kernel times) of a context.  The table is read first, so the DUMP
    instantiation of the count kernel is the one that finds the regions above 65535 and hands them to the table; the
    voting instantiation then meets them already flagged (read_results_first is the other order)."""
    table = kc.dump_table()
    res = kc.sorted_results()
    return table, res, kc.stats(), kc.kernel_times()


def read_results_first(kc):
    """(sorted results, stats, kernel times) with no dump_table() before: the voting instantiation of the count kernel
    decides by itself which regions fit the 16-bit counters, and kc_finalize moves the others to the table"""
    res = kc.sorted_results()
    return res, kc.stats(), kc.kernel_times()


def check_path(kt, path, flagged):
    # FLAGGED is also the name under which kernel_times() reports kc_l1_to_table_kernel, the drain of a full buffer into
    # the table (bk_drain_t in kc_api.hip).  No buffer fills up in the tests that come here (the two-pass tests, which
    # do fill one, make room by a spill and assert their own path), so a launch under this name is a flagged region.
    if path == "table":
        assert EXTRACT_INSERT in kt and "kc_count_kernel" not in kt and FLAGGED not in kt, kt
    else:
        assert "kc_count_kernel" in kt and EXTRACT_INSERT not in kt, kt
        assert (FLAGGED in kt) == flagged, kt


# ---- the vote at its thresholds ----------------------------------------------------------------------
@pytest.mark.parametrize("dmin_thres", [1, 2, 3, 5])
@pytest.mark.parametrize("path", list(PATHS))
def test_vote_grid(path, dmin_thres):
    k, tuning = PATHS[path]
    cases, blocks = family("grid", k, dmin_thres)
    ores, otable, ost, _, _ = oracle_of("grid", k, dmin_thres, cases, blocks)
    with pkg.KmerCounter(k, dmin_thres=dmin_thres, tuning=tuning or None, time_kernels=True) as kc:
        kc.submit_reads(*blocks[0])  # one submission holds the whole grid
        kc.flush()
        table, res, st, kt = read_out(kc)
    same(table, CC.expected_table(cases), "table vs construction")
    same(table, otable, "table vs oracle")
    same(res, CC.expected_results(cases, dmin_thres), "results vs construction")
    same(res, ores, "results vs oracle")
    check_stats(st, cases, dmin_thres, ost)
    check_path(kt, path, flagged=False)


# ---- the 16-bit halves at 65535 ----------------------------------------------------------------------
@pytest.mark.parametrize("n", CC.SATURATION_NS)
@pytest.mark.parametrize("path", BUCKETED)
def test_saturation(path, n):
    """One k-mer, hence one region, of exactly n records per submission: up to 65535 the LDS table counts it (no half
    may carry into its neighbour), from 65536 on the global table takes the region whole.  Every submission is read out
    in both orders, so that each instantiation of the count kernel makes that decision once by itself."""
    k, tuning = PATHS[path]
    mine = saturation_cases(k, n)
    assert len(mine) == 4
    with pkg.KmerCounter(k, tuning=dict(tuning, **LONG_CHAINS), time_kernels=True) as kc:
        for c, block in mine:
            # the oracle saw exactly this submission: its table, results and stats are this submission's
            ores, otable, ost, _, _ = oracle_of("saturation n=%d split=%d" % (n, c.tags["split"]), k, 2, [c], [block])
            # results first: the voting instantiation itself keeps the region in LDS or sends it to the table ...
            kc.reset()
            kc.kernel_times(clear=True)
            kc.submit_reads(*block)
            kc.flush()
            res, st, kt = read_results_first(kc)
            same(res, CC.expected_results([c], 2), c.name + ": results vs construction, results first")
            same(res, ores, c.name + ": results vs oracle, results first")
            check_stats(st, [c], 2, ost)
            check_path(kt, path, flagged=n > 65535)
            # ... and the table first: the DUMP instantiation does
            kc.reset()
            kc.kernel_times(clear=True)
            kc.submit_reads(*block)
            kc.flush()
            table, res, st, kt = read_out(kc)
            same(table, CC.expected_table([c]), c.name + ": table vs construction")
            same(table, otable, c.name + ": table vs oracle")
            same(res, CC.expected_results([c], 2), c.name + ": results vs construction")
            same(res, ores, c.name + ": results vs oracle")
            check_stats(st, [c], 2, ost)
            check_path(kt, path, flagged=n > 65535)


@pytest.mark.parametrize("n", [65535, 65536])
@pytest.mark.parametrize("path", ["wide", "two-word-33", "two-word-51", "n-word-77", "n-word-125"])
def test_region_fill(path, n):
    """One region in all (p1 = p2 = 1; compact records need a bit of each fan-out): three k-mers share it, and the
    region, not any one of them, sits on the boundary."""
    k, tuning = PATHS[path]
    cases, blocks = family("fill", k, n=n)
    ores, otable, ost, _, _ = oracle_of("fill-%d" % n, k, 2, cases, blocks)
    with pkg.KmerCounter(k, tuning=dict(tuning, p1=1, p2=1, **LONG_CHAINS), time_kernels=True) as kc:
        kc.submit_reads(*blocks[0])
        kc.flush()
        table, res, st, kt = read_out(kc)
    same(table, CC.expected_table(cases), "table vs construction")
    same(table, otable, "table vs oracle")
    same(res, CC.expected_results(cases, 2), "results vs construction")
    same(res, ores, "results vs oracle")
    check_stats(st, cases, 2, ost)
    check_path(kt, path, flagged=n > 65535)


# ---- sums across buffer passes -----------------------------------------------------------------------
def check_two_pass(k, table, res, st, cases, blocks, with_raw=True):
    ores, otable, ost, _, _ = oracle_of("two-pass", k, 2, cases, blocks)
    same(table, CC.expected_table(cases), "table vs construction")
    same(table, otable, "table vs oracle")
    same(res, CC.expected_results(cases, 2), "results vs construction")
    same(res, ores, "results vs oracle")
    check_stats(st, cases, 2, ost, raw=with_raw)


TWO_PASS = [("default", None), ("compact", None), ("compact", "0"), ("compact-short", None), ("compact-short", "0"), ("wide", None),
            ("two-word-33", None), ("two-word-51", None), ("n-word-77", None), ("n-word-125", None)]


@pytest.mark.parametrize("path,light_spill", TWO_PASS, ids=["%s%s" % (p, "-merged" if e else "") for p, e in TWO_PASS])
def test_two_pass(path, light_spill, monkeypatch):
    """A buffer that holds one block but not two: a k-mer's counters of the two passes are added in the global table
    (clipped when they are read out), or -- compact records, KC_LIGHT_SPILL not 0 -- its records of both passes meet in
    level 2 and the region goes to the table when it has outgrown 65535."""
    if light_spill is not None:
        monkeypatch.setenv("KC_LIGHT_SPILL", light_spill)
    else:
        monkeypatch.delenv("KC_LIGHT_SPILL", raising=False)
    k, tuning = PATHS[path]
    cases, blocks = family("two-pass", k)
    sizes = [len(b[2]) - 1 for b in blocks]
    cap = max(sizes) + 1000
    assert len(blocks) == 2 and cap < sum(sizes)
    with pkg.KmerCounter(k, max_kmers_buffered=cap, tuning=dict(tuning, **SMALL_BUFFER), time_kernels=True) as kc:
        for b in blocks:
            kc.submit_reads(*b)
        kc.flush()
        table, res, st, kt = read_out(kc)
    check_two_pass(k, table, res, st, cases, blocks)
    assert "kc_count_kernel" in kt and EXTRACT_INSERT not in kt and l2_launches(kt) >= 2, kt
    light = path.startswith("compact") and light_spill is None
    if light:
        # the regions of 80000 and 65536 records outgrew the LDS counters: the table took them
        assert FLAGGED in kt, kt
    else:
        # the first pass was counted and merged into the table; no region of either pass outgrew the LDS counters
        assert kt.get(MERGE, (0, 0.0))[0] >= 1 and FLAGGED not in kt, kt


def _union_tables(parts):
    keys = np.concatenate([p[0] for p in parts])
    order = np.lexsort([keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)])
    return tuple(np.concatenate([p[i] for p in parts])[order] for i in range(len(parts[0])))


@pytest.mark.parametrize("path", ["compact", "two-word-51"])
def test_two_pass_as_records_of_two_shards(path):
    """The same reads as one block through kc_extract_partition -> kc_insert_records, two shards on one device: the count
    kernel behind another record format."""
    import torch
    k, tuning = PATHS[path]
    cases, blocks = family("two-pass", k)
    b, q = np.concatenate([x[0] for x in blocks]), np.concatenate([x[1] for x in blocks])
    total = len(b) // (k + 2)
    offs = np.arange(total + 1, dtype=np.uint64) * np.uint64(k + 2)
    R = 2
    shards = [pkg.KmerCounter(k, rank_me=r, rank_n=R, tuning=dict(tuning, **LONG_CHAINS), time_kernels=True) for r in range(R)]
    nl = shards[0].rec_nl
    recs = torch.zeros(R * total * nl, dtype=torch.int64, device="cuda")
    counts = shards[0].extract_partition(b, q, offs, recs, total)
    assert int(counts.sum()) == total
    outs = []
    for d in range(R):
        shards[d].insert_records(recs[d * total * nl:], int(counts[d]))
        shards[d].flush()
        outs.append(read_out(shards[d]))
    for s in shards:
        s.close()
    st = {f: sum(o[2][f] for o in outs) for f in outs[0][2]}
    check_two_pass(k, _union_tables([o[0] for o in outs]), _union_tables([o[1] for o in outs]), st, cases, blocks, with_raw=False)
    for d in range(R):
        if int(counts[d]):
            assert "kc_count_kernel" in outs[d][3] and EXTRACT_INSERT not in outs[d][3], outs[d][3]
    assert any(FLAGGED in o[3] for o in outs)  # the regions of 80000 and 65536 records


@pytest.mark.parametrize("path", ["compact", "two-word-51"])
def test_two_pass_through_the_shard_flow(path):
    """... and through the single-pass shard flow (kc_shard_extract / kc_shard_reserve / kc_shard_commit), R = 2."""
    from test_gpu_shard_flow import run_shards
    k, tuning = PATHS[path]
    cases, blocks = family("two-pass", k)
    reads, quals = [], []
    for b, q, _ in blocks:
        r, ql = CC.read_strings(b, q, k)
        reads += r
        quals += ql
    shards, shipped, total = run_shards(reads, quals, k, 2, dict(tuning, **LONG_CHAINS), blocks=1, time_kernels=True)
    assert shipped > 0 and total == len(reads)
    outs = [read_out(s) for s in shards]
    for s in shards:
        s.close()
    st = {f: sum(o[2][f] for o in outs) for f in outs[0][2]}
    check_two_pass(k, _union_tables([o[0] for o in outs]), _union_tables([o[1] for o in outs]), st, cases, blocks, with_raw=False)
    assert any("kc_count_kernel" in o[3] for o in outs)
    assert all(EXTRACT_INSERT not in o[3] for o in outs)
    assert any(FLAGGED in o[3] for o in outs)  # the regions of 80000 and 65536 records


# ---- lookup ------------------------------------------------------------------------------------------
def _lookup_matches(kc, cases, dmin_thres):
    keys = np.array([c.key for c in cases], dtype=np.uint64).reshape(len(cases), -1)
    other = np.stack([O.revcomp(kk, kc.k) for kk in keys])
    for q in (keys, other):  # either strand finds the entry
        cnt, left, right = kc.lookup(q)
        for i, c in enumerate(cases):
            want = c.result(dmin_thres) or (0, None, None)
            assert int(cnt[i]) == want[0], c.name
            if want[0]:
                assert (chr(left[i]), chr(right[i])) == want[1:], c.name


def test_lookup_of_saturated_and_threshold_kmers():
    """lookup() finalizes by itself (no dump_table() before it), so here too the voting instantiation decides alone what
    fits the LDS counters.  A context per n holds the two splits that survive S8: 131 070 and 131 072 reads."""
    k, _ = PATHS["default"]
    for n in (65535, 65536):
        mine = [c for c, _ in saturation_cases(k, n) if c.result(2)]
        assert [c.tags["split"] for c in mine] == [0, 1]
        with pkg.KmerCounter(k, tuning=LONG_CHAINS) as kc:
            kc.submit_reads(*CC.emit(mine, k, 3000 + n))
            kc.flush()
            _lookup_matches(kc, mine, 2)
    for dmin_thres in (2, 5):
        cases, blocks = family("grid", k, dmin_thres)
        at = [c for c in cases if c.tags["c"] in (40, 100)]
        assert any(c.result(dmin_thres) for c in at) and any(not c.result(dmin_thres) for c in at)
        with pkg.KmerCounter(k, dmin_thres=dmin_thres) as kc:
            kc.submit_reads(*blocks[0])
            kc.flush()
            _lookup_matches(kc, cases, dmin_thres)
