"""kc_merge_pairs and kc_trim_adapters compared exactly at sizes where their scans carry between rounds: more than
1 048 576 pairs (two rounds of 8192 tiles of 64 pairs) and more than 2 097 152 reads (one round of tiles of 256 reads).

The models cannot run at that size, and need not: both steps are independent per pair (per read when unpaired), so the
expected bytes, offsets and counters of an arrangement of already-modelled items are a numpy gather of the per-item
results (MergeItems.compose, TrimItems.compose; tests/test_frontend_compose.py pins them against the models).  The
arrangements put long pairs at the first and the last place of a tile, side by side, across a tile's border, into a tile
of their own and into the last, partial tile, put a tile of dropped pairs in, and place the longest pairs behind each
round of the scan.

Wall time on the MI355X run: the merge base set (about 31 000 pairs) took the model 5 s, the trim base set (10 077
pairs) 12 s per score set; composing 1 100 037 pairs took 2.7 s and the device call 0.08 s, composing 2 200 014 reads
3.2 s and the device call 0.05 s with device input, 0.06 s with host input; the chain's oracle 8.9 s.  The module as a
whole ran in about 80 s."""
import json
import os
import time

import numpy as np
import pytest

import merge_model as MM
import mhm2_kmer_analysis_v2_amd as pkg
import trim_model as TM

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FA_PATH = os.path.join(HERE, "golden", "adapters_no_transposase.fa")
FA = open(FA_PATH, "rb").read()
FA_SEQS = TM.read_fasta_seqs(FA_PATH)
MSTATS = ("pairs", "merged", "ambiguous", "dropped", "overlap_len", "merged_len", "out_reads", "out_bases")
TILE = 64
_cache = {}


def merge_base():
    """at least 30 000 distinct pairs: random ones, every family of merge_model.py, every hand case"""
    if "merge" not in _cache:
        t0 = time.time()
        cases = json.load(open(os.path.join(HERE, "golden", "merge_hand_cases.json")))["cases"]
        pairs = MM.random_pairs(np.random.default_rng(101), 23000, 1, 300)
        pairs += MM.length_grid_pairs() + MM.cross_chunk_pairs() + MM.long_path_pairs()
        pairs += [tuple(x.encode() for x in c["pair"]) for c in cases if c["qual_offset"] == 33]
        pairs += MM.random_pairs(np.random.default_rng(102), 1500, 1, 20)  # mostly dropped
        pairs = list(dict.fromkeys(pairs))
        items = MM.MergeItems(pairs)
        _cache["merge"] = (items, time.time() - t0)
    return _cache["merge"]


def merge_arrangement(items, m, seed):
    """A seeded arrangement of m pairs (m not a multiple of 64) with the long and the dropped pairs placed on purpose."""
    assert m % TILE and m > 400 * TILE
    rng = np.random.default_rng(seed)
    long = items.is_long()
    giant = np.nonzero(np.maximum(items.len1, items.len2) > 2000)[0]
    longs = np.nonzero(long & (np.maximum(items.len1, items.len2) <= 2000))[0]
    shorts = np.nonzero(~long)[0]
    dropped = np.nonzero(items.stats[:, 2] == 1)[0]
    order = rng.choice(shorts, m)
    at = rng.choice(m, m // 100, replace=False)  # one pair in a hundred is long
    order[at] = rng.choice(longs, len(at))
    # Placements on purpose.  Each takes a full tile of its own (drawn without replacement, none of them the first or
    # the last two), and the single spots further down lie in tiles 0, 4687 and 8193, 16385: nothing overwrites another.
    ntiles = (m + TILE - 1) // TILE
    reserved = {0, 300000 // TILE, (300000 + len(giant)) // TILE} | {r * 8192 + 1 for r in range(1, 4)}
    free = np.array([t for t in range(1, ntiles - 2) if t not in reserved])
    all_long, all_dropped, first, last, beside, border = (int(x) * TILE for x in rng.choice(free, 6, replace=False))
    order[all_long:all_long + TILE] = rng.choice(longs, TILE)       # a tile of long pairs only
    order[all_dropped:all_dropped + TILE] = rng.choice(dropped, TILE)  # a tile that writes nothing
    order[first] = longs[0]                                         # first of a tile
    order[last + TILE - 1] = longs[1]                               # last of a tile
    order[beside + 5:beside + 8] = longs[2:5]                       # side by side
    order[border + TILE - 1:border + TILE + 1] = longs[5:7]         # across a border (the next tile may be a placed one: the asserts below hold either way)
    order[m - 1] = longs[7]                                         # in the last, partial tile
    order[m - 3] = giant[0]
    # the longest pairs: in the first tile, and behind every round of the scan (8192 tiles = 524 288 pairs)
    spots = [3] + [r * 524288 + 70 for r in range(1, m // 524288 + 1) if r * 524288 + 70 < m - 4]
    for n, s in enumerate(spots):
        order[s] = giant[n % len(giant)]
        order[s + 1] = giant[(n + 1) % len(giant)]
    if m > 600000:
        order[300000:300000 + len(giant)] = giant                  # each of them once
    lo = long[order]
    tiles = lo[:m // TILE * TILE].reshape(-1, TILE)
    assert tiles.all(axis=1).any() and tiles[:, 0].any() and tiles[:, -1].any() and (lo[1:] & lo[:-1]).any()
    assert lo[m // TILE * TILE:].any()
    dr = items.stats[order, 2] == 1
    assert dr[:m // TILE * TILE].reshape(-1, TILE).all(axis=1).any()
    return order


def first_difference(got, want):
    """index of the first element that differs (the shorter length when one array is a prefix of the other), or None"""
    n = min(len(got), len(want))
    d = np.nonzero(got[:n] != want[:n])[0]
    if len(d):
        return int(d[0])
    return None if len(got) == len(want) else n


def first_bad_pair(items, order, got_o, want_o, got_p, want_p):
    """index of the first pair whose offsets or bytes differ, for the message"""
    reads_upto = np.cumsum(items.out_nreads[order])  # output reads of the pairs 0 .. p
    bytes_upto = np.cumsum(items.out_bytes[order])
    bad = len(order)
    entry = first_difference(got_o, want_o)  # offsets[r + 1] closes read r
    if entry is not None:
        bad = min(bad, int(np.searchsorted(reads_upto, max(entry - 1, 0), side="right")))
    byte = first_difference(got_p, want_p)
    if byte is not None:
        bad = min(bad, int(np.searchsorted(bytes_upto, byte, side="right")))
    return bad


def run_merge(items, order, device_input, what, kc=None):
    import torch
    t0 = time.time()
    b, q, o, want_p, want_o, want_st = items.compose(order)
    t1 = time.time()
    own = kc is None
    kc = kc or pkg.KmerCounter(21)
    try:
        if device_input:
            args = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (b, q, o)]
        else:
            args = [b, q, o]
        torch.cuda.synchronize()
        t2 = time.time()
        packed, offs, st = kc.merge_pairs(*args, min_kmer_len=21)
        torch.cuda.synchronize()
        t3 = time.time()
        got_p, got_o = packed.cpu().numpy(), offs.cpu().numpy().view(np.uint64)
    finally:
        if own:
            kc.close()
    nlong = int(items.is_long()[order].sum())
    print("%s: %d pairs in %d tiles, %d long pairs, %d input bases; compose %.1f s, device %.2f s; %s"
          % (what, len(order), (len(order) + TILE - 1) // TILE, nlong, len(b), t1 - t0, t3 - t2, want_st))
    assert nlong > 0
    same = len(got_o) == len(want_o) and len(got_p) == len(want_p) and np.array_equal(got_o, want_o) and np.array_equal(got_p, want_p)
    if not same:
        p = first_bad_pair(items, order, got_o, want_o, got_p, want_p)
        item = int(order[min(p, len(order) - 1)])
        pytest.fail("%s: output differs first at pair %d (tile %d, place %d of it; base item %d, mates of %d and %d, long: %s)"
                    % (what, p, p // TILE, p % TILE, item, items.len1[item], items.len2[item], bool(items.is_long()[item])))
    assert {s: st[s] for s in MSTATS} == want_st
    return packed, offs, (want_p, want_o, want_st)


def test_merge_base_set():
    items, secs = merge_base()
    lo = items.is_long()
    print("merge base set: %d pairs, %d long, %d dropped, %d Ns, model %.1f s"
          % (len(items), lo.sum(), (items.stats[:, 2] == 1).sum(), (items.bases == MM.N).sum(), secs))
    assert len(items) >= 30000 and lo.sum() >= 200 and (items.stats[:, 2] == 1).sum() >= 500
    assert ((items.bases == MM.N).sum()) > 1000 and items.stats[:, 0].sum() > 10000 and (items.stats[:, 1] > 0).sum() > 1000


@pytest.mark.parametrize("device_input", [True, False])
def test_merge_1_100_037_pairs(device_input):
    items, _ = merge_base()
    m = 1_100_037
    assert m > 2 * 8192 * TILE and m % TILE
    order = merge_arrangement(items, m, 7)
    run_merge(items, order, device_input, "merge, %s input" % ("device" if device_input else "host"))


def test_merge_small_arrangements_share_a_counter():
    """the scratch arrays and the staged block are reused from call to call: a large call, a small one, a large one"""
    items, _ = merge_base()
    with pkg.KmerCounter(21) as kc:
        for m, dev in ((70_001, True), (451, False), (70_001, False), (1_037, True)):
            run_merge(items, merge_arrangement(items, m, m) if m > 400 * TILE else np.random.default_rng(m).integers(0, len(items), m),
                      dev, "merge of %d" % m, kc)


def test_chain_of_a_composed_arrangement_matches_oracle():
    from oracle import cpu_oracle as O
    items, _ = merge_base()
    m = 160_003
    order = merge_arrangement(items, m, 9)
    with pkg.KmerCounter(21) as kc:
        packed, offs, (want_p, want_o, want_st) = run_merge(items, order, True, "chain", kc)
        assert want_st["out_reads"] > 150_000
        kc.submit_packed_reads(packed, offs, nreads=want_st["out_reads"])  # the device output as it is
        kc.flush()
        gk, gc, gl, gr = kc.sorted_results()
    ab, aq, ao = MM.packed_to_ascii(want_p, want_o)
    t0 = time.time()
    orc = O.Oracle(21, nranks=1, nthreads=8)
    orc.add_reads(ab, aq, ao)
    ok, oc, ol, orr = orc.finalize()
    print("chain: %d reads, %d bases, %d k-mers, oracle %.1f s" % (want_st["out_reads"], want_st["out_bases"], len(oc), time.time() - t0))
    assert gk.shape == ok.shape and (gk == ok).all()
    assert (gc == oc).all() and (gl == ol).all() and (gr == orr).all()


# ---- trim ------------------------------------------------------------------------------------------------------------------
def trim_base(blastn, npairs):
    key = ("trim", blastn, npairs)
    if key not in _cache:
        t0 = time.time()
        ads = TM.AdapterSet(FA, 21, blastn)
        b, q, o = TM.random_pairs(500 + blastn, npairs, FA_SEQS)
        long_ad = [s for s in FA_SEQS if len(s) >= 60][0]
        fam = [r for r, _, _ in TM.seed_position_reads(ads, long_ad, seed=81)]
        rng = np.random.default_rng(82)
        fam += ["", "A", long_ad[:40], long_ad[:20]]
        fam += fam[:1 - len(fam) % 2]  # an odd count so far: the last of the next five is mate 2 of its pair
        fam += [TM._no_seed_filler(rng, ads, 4 * m) + long_ad[:21] for m in (0, 1, 13, 56, 57)]  # seed in the last k-mer
        tail_read = 2 * npairs + len(fam) - 1  # 4 * 57 + 21 bases, 1 (mod 4): its last word holds one byte
        assert tail_read % 2 == 1 and len(fam) % 2 == 0
        fb, fq, fo = TM.reads_to_arrays(fam, seed=83)
        b, q = np.concatenate([b, fb]), np.concatenate([q, fq])
        o = np.concatenate([o, fo[1:] + o[-1]])
        items = TM.TrimItems(ads, b, q, o)
        assert items.len[tail_read] == 4 * 57 + 21 and items.naligns[tail_read] == 1
        _cache[key] = (items, time.time() - t0, tail_read)
    return _cache[key]


def run_trim(items, order, paired, blastn, what, device_input=True):
    import torch
    t0 = time.time()
    b, q, o, wb, wq, wo, wst = items.compose(order, paired)
    t1 = time.time()
    with pkg.KmerCounter(21) as kc:
        kc.load_adapters(FA, 21, blastn)
        args = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (b, q, o)] if device_input else [b, q, o]
        torch.cuda.synchronize()
        t2 = time.time()
        gb, gq, go, gst = kc.trim_adapters(*args, paired=paired)
        torch.cuda.synchronize()
        t3 = time.time()
        gb, gq, go = gb.cpu().numpy(), gq.cpu().numpy(), go.cpu().numpy()
    nreads = len(o) - 1
    print("%s: %d reads in %d tiles of 256, %d input bases; compose %.1f s, device %.2f s; %s"
          % (what, nreads, (nreads + 255) // 256, len(b), t1 - t0, t3 - t2, wst))
    if not np.array_equal(go, wo):
        r = int(np.nonzero(go != wo)[0][0]) - 1
        pytest.fail("%s: offsets differ first behind read %d (tile %d, place %d): %d != %d" % (what, r, r // 256, r % 256, go[r + 1], wo[r + 1]))
    for name, g, w in (("bases", gb, wb), ("qualities", gq, wq)):
        if not np.array_equal(g, w):
            at = int(np.nonzero(g != w)[0][0]) if len(g) == len(w) else min(len(g), len(w))
            r = int(np.searchsorted(wo, at, side="right")) - 1
            pytest.fail("%s: %s differ first in read %d (tile %d)" % (what, name, r, r // 256))
    assert gst == wst, (what, gst, wst)
    return wst


@pytest.mark.parametrize("device_input", [True, False])
@pytest.mark.parametrize("paired", [True, False])
def test_trim_2_200_000_reads(paired, device_input):
    items, secs, tail_read = trim_base(False, 10000)
    npairs = len(items.len) // 2
    assert npairs >= 10000
    print("trim base set: %d pairs, model %.1f s" % (npairs, secs))
    rng = np.random.default_rng(11 + paired)
    nreads = 2_200_014 if paired else 2_200_013
    assert nreads > 8192 * 256 and nreads % 256 and nreads % 128 and nreads % 32
    order = rng.integers(0, npairs if paired else 2 * npairs, nreads // 2 if paired else nreads)
    order[-1] = tail_read // 2 if paired else tail_read  # the input ends with a read whose only seed is its last k-mer
    st = run_trim(items, order, paired, False, "trim, paired=%s, %s input" % (paired, "device" if device_input else "host"), device_input)
    assert st["trimmed"] > 400_000 and st["reads_removed"] > 0


@pytest.mark.parametrize("paired", [True, False])
def test_trim_other_scores_150_000_reads(paired):
    items, secs, _ = trim_base(True, 3000)
    npairs = len(items.len) // 2
    rng = np.random.default_rng(13 + paired)
    nreads = 150_030 if paired else 150_029
    order = rng.integers(0, npairs if paired else 2 * npairs, nreads // 2 if paired else nreads)
    st = run_trim(items, order, paired, True, "trim, 2/3 scores, paired=%s" % paired, device_input=not paired)
    assert st["trimmed"] > 20_000
