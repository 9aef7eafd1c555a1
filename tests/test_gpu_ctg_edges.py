"""The contig k-mer pass (kc_begin_ctg_kmers, kc_submit_ctg_block, kc_ctg_insert_kernel, kc_ctg_merge_kernel and the owner
branch of csrc/kc_ctg.hpp) on contigs whose outcome is known by construction (tests/ctg_cases.py): the decision table of
read entry x contig occurrences row by row, dmin_thres above 2, every key width, palindromes, the shape of a submission,
the seams between the launches of one block, and the one owner of a k-mer on every route of a context of several ranks.
Everything is compared for equality with the construction AND with the oracle.  Need a real MI355X."""
import numpy as np
import pytest

import ctg_cases as G
import mhm2_kmer_analysis_v2_amd as pkg
from oracle import cpu_oracle as O
from test_gpu_count_edges import same

pytestmark = pytest.mark.gpu

KS = [21, 30, 31, 32, 33, 63, 64, 95, 125]
PATHS = {"bucketed": None, "table": dict(mode=1)}
ROOM = 1 << 16  # distinct contig k-mers kc_begin_ctg_kmers makes room for, where the test is not about that room

_sets = {}


def case_set(name, k):
    """(cases, reads, contigs, depths) of a case set, built once"""
    if (name, k) not in _sets:
        cases = G.families(k) if name == "families" else G.seam_cases(k, 2500)
        ctgs, depths = G.emit_ctgs(cases, seed=7)
        _sets[name, k] = (cases, G.emit_reads(cases, k, 31), ctgs, depths)
    return _sets[name, k]


_oracle = {}


def oracle_of(name, k, dmin_thres):
    """the oracle's sorted results for a case set: once per (set, k, dmin_thres)"""
    if (name, k, dmin_thres) not in _oracle:
        _, reads, ctgs, depths = case_set(name, k)
        o = O.Oracle(k, dmin_thres=dmin_thres, nranks=3, nthreads=2)
        o.add_reads(*reads)
        for c, d in zip(ctgs, depths):
            o.add_ctg(c, d)
        _oracle[name, k, dmin_thres] = o.finalize()
        assert o.stats()["dropped"] == 0
        o.close()
    return _oracle[name, k, dmin_thres]


def submit(kc, ctgs, depths, shape):
    if shape == "block":
        kc.submit_ctgs(ctgs, depths)
    elif shape == "each":
        for c, d in zip(ctgs, depths):
            kc.submit_ctgs([c], [d])
    elif shape == "halves":  # in another order than the block's
        order = np.random.default_rng(5).permutation(len(ctgs))
        half = len(order) // 2
        for part in (order[:half], order[half:]):
            kc.submit_ctgs([ctgs[i] for i in part], [depths[i] for i in part])
    elif shape == "device":  # the sequence at an odd address, the depths 2-byte but not 4-byte aligned
        import torch
        block, dd = G.as_block(ctgs, depths)
        n = len(block)
        sbuf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        dbuf = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
        sbuf[1:1 + n] = torch.from_numpy(block.copy()).cuda()
        dbuf[1:1 + n] = torch.from_numpy(dd.view(np.int16).copy()).cuda()
        seq, dep = sbuf[1:1 + n], dbuf[1:1 + n]
        assert seq.data_ptr() % 2 == 1 and dep.data_ptr() % 4 == 2
        torch.cuda.synchronize()  # the copies ran on torch's stream, the context has a stream of its own
        kc.submit_ctg_block(seq, dep)
    else:
        raise ValueError(shape)


def run(name, k, dmin_thres, tuning, shape="block", room=ROOM):
    """(sorted results, stats, ctg_stats, kernel launches of the contig submissions) of one context"""
    cases, reads, ctgs, depths = case_set(name, k)
    with pkg.KmerCounter(k, dmin_thres=dmin_thres, tuning=tuning) as kc:
        kc.submit_reads(*reads)
        kc.begin_ctg_kmers(room)
        before = kc.stats()["num_gpu_calls"]
        submit(kc, ctgs, depths, shape)
        launches = kc.stats()["num_gpu_calls"] - before
        return kc.sorted_results(), kc.stats(), kc.ctg_stats(), launches


def check(name, k, dmin_thres, res, st, cst):
    cases = case_set(name, k)[0]
    same(res, G.expected_results(cases, dmin_thres), "results vs construction")
    same(res, oracle_of(name, k, dmin_thres), "results vs oracle")
    est = G.expected_stats(cases, dmin_thres)
    assert (st["total_kmers"], st["sum_counts"]) == (est["total_kmers"], est["sum_counts"])
    assert st["kmers_inserted"] == sum(c.reads.occurrences for c in cases) and st["num_dropped"] == 0
    assert cst == G.expected_ctg_stats(cases)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("dmin_thres", G.DMIN_THRES)
@pytest.mark.parametrize("k", KS)
def test_every_family(k, dmin_thres, path):
    """The rows with dmin_thres 3 and 5 and a smallest depth in [2, dmin_thres) are the ones a literal 2 in
    kc_ctg_merge_kernel keeps and the reference does not."""
    res, st, cst, _ = run("families", k, dmin_thres, PATHS[path])
    check("families", k, dmin_thres, res, st, cst)


@pytest.mark.parametrize("k", [21, 64])
def test_the_shape_of_a_submission_does_not_matter(k):
    dmin_thres = 3
    first = None
    for shape in ("block", "each", "halves", "device"):
        res, st, cst, launches = run("families", k, dmin_thres, None, shape=shape)
        check("families", k, dmin_thres, res, st, cst)
        assert launches == {"block": 1, "each": len(case_set("families", k)[2]), "halves": 2, "device": 1}[shape]
        if first is None:
            first = (res, cst)
        else:
            same(res, first[0], shape + " vs block")
            assert cst == first[1]


@pytest.mark.parametrize("k", [21, 33])
def test_a_block_taken_in_many_launches_counts_every_window_once(k):
    """A table of 4096 slots whose free room under three quarters is far smaller than the block: kc_submit_ctg_block cuts the
    block wherever the room ends -- the room shrinks from launch to launch, so the cuts fall inside contigs and windows --
    and every window is still counted exactly once."""
    cases, _, ctgs, _ = case_set("seam", k)
    distinct, positions = G.expected_ctg_stats(cases)
    assert distinct == len(cases) == 2500 and distinct < 4096 * 3 // 4 < positions // 8
    one = run("seam", k, 2, None, room=positions)  # room for a k-mer at every position: one launch
    check("seam", k, 2, *one[:3])
    assert one[3] == 1
    many = run("seam", k, 2, None, room=2048)  # -> 4096 slots
    check("seam", k, 2, *many[:3])
    assert many[3] >= 8
    same(many[0], one[0], "many launches vs one")
    assert many[2] == one[2]


# ---- one owner per k-mer on every route ----------------------------------------------------------------
ROUTES = [("hash", 21), ("hash", 31), ("hash", 51), ("reference", 21), ("reference", 51), ("shard-flow", 21), ("shard-flow", 51),
          ("wire-units", 21), ("wire-units", 33)]
_owner_inputs = {}


def owner_inputs(k):
    """reads, contigs and the oracle's answers with and without the contigs: once per k"""
    if k not in _owner_inputs:
        from test_gpu_ctg import make_ctgs
        rng = np.random.default_rng(1700 + k)
        genome = "".join(rng.choice(list("ACGT"), size=3000))
        reads, quals = [], []
        for _ in range(700):
            a = int(rng.integers(0, len(genome) - 160))
            ln = int(rng.integers(k + 2, 150))
            reads.append(genome[a:a + ln])
            quals.append("I" * ln)
        ctgs, depths = make_ctgs(rng, genome, k)
        # one read out of the contig that no other read covers: singleton read entries that contig k-mers meet
        reads.append(ctgs[-1][100:100 + k + 40])
        quals.append("I" * (k + 40))
        b, q, offs = O.reads_to_arrays(reads, quals)
        o = O.Oracle(k, nranks=3, nthreads=1)
        o.add_reads(b, q, offs)
        table = o.dump_table()
        plain = o.finalize()
        o.close()
        o = O.Oracle(k, nranks=3, nthreads=1)
        o.add_reads(b, q, offs)
        for c, d in zip(ctgs, depths):
            o.add_ctg(c, d)
        want = o.finalize()
        o.close()
        # the contigs' k-mers meet a kept read entry, a singleton read entry, and no read entry at all
        kept = {tuple(int(x) for x in w) for w in plain[0]}
        single = {tuple(int(x) for x in w) for w, n in zip(table[0], table[1]) if n == 1}
        seen = {tuple(int(x) for x in w) for w in table[0]}
        comp = str.maketrans("ACGT", "TGCA")
        ctg_keys = set()
        for c in ctgs:
            for i in range(1, len(c) - k):
                w = c[i:i + k]
                if set(c[i - 1:i + k + 1]) <= set("ACGT"):
                    ctg_keys.add(tuple(int(x) for x in O.pack_kmer(min(w, w[::-1].translate(comp)))))
        assert ctg_keys & kept and ctg_keys & single and ctg_keys - seen
        added = {tuple(int(x) for x in w) for w in want[0]} - kept
        assert added & single and added - seen
        _owner_inputs[k] = (reads, quals, (b, q, offs), ctgs, depths, want, added)
    return _owner_inputs[k]


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("route,k", ROUTES)
def test_every_route_keeps_a_contig_kmer_on_the_one_rank_that_owns_it(route, k, R):
    """Every rank is given every contig.  The union of the ranks' results is the oracle's single answer, no key sits on two
    ranks, and every result -- the contigs' additions included -- sits where the route's owner function says: the hash,
    the reference's target rank, the level-1 bucket of the shard flow, and the owner bits of the wire units (k = 21 with
    1024 level-1 buckets; at k = 33 the flag changes nothing and the hash decides)."""
    reads, quals, arrays, ctgs, depths, want, added = owner_inputs(k)
    room = sum(len(c) for c in ctgs)
    if route == "shard-flow":
        from test_gpu_shard_flow import run_shards
        shards, _, _ = run_shards(reads, quals, k, R, None)
    elif route == "wire-units":
        from test_gpu_wire6 import SHORT, run_flow
        shards, (uw, ur, Q), _ = run_flow(reads, quals, k, R, SHORT if k == 21 else None)
        assert (uw, ur) == ((3, 4) if k == 21 else (shards[0].rec_nl, 1))  # wire units are active exactly at k = 21
    else:
        shards = [pkg.KmerCounter(k, rank_me=r, rank_n=R, reference_owner=(route == "reference")) for r in range(R)]
        for s in shards:
            s.submit_reads(*arrays)
    try:
        parts = []
        for s in shards:
            s.begin_ctg_kmers(room)
            s.submit_ctgs(ctgs, depths)
            parts.append(s.sorted_results())
        keys = np.concatenate([p[0] for p in parts])
        order = np.lexsort([keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)])
        got = tuple(np.concatenate([p[i] for p in parts])[order] for i in range(4))
        assert len(np.unique(keys, axis=0)) == len(keys)  # no key on two ranks
        same(got, want, "union vs oracle")
        n_added = 0
        for r, (s, p) in enumerate(zip(shards, parts)):
            owner = s.shard_owner if route == "shard-flow" else s.partition_owner
            for i in range(len(p[1])):
                is_added = tuple(int(x) for x in p[0][i]) in added
                n_added += is_added
                if is_added or i % 7 == 0:
                    assert owner(p[0][i]) == r, (r, i, is_added)
        assert n_added == len(added)
    finally:
        for s in shards:
            s.close()
