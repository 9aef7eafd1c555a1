"""kc_aln_depths (csrc/kc_depth.hpp) against the host model tests/depth_model.py, byte for byte: the depths, the contigs'
records and the statistics on the same inputs.  The model is never replaced by a second device run.

Every device call goes through device_depths: the records and both outputs in device arrays of exactly their size inside
canaries.  The call's validity does not look at reads, so the records are forged and no alignment runs here (the chain
test at the end excepted)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_model as A
import depth_model as D
import mhm2_kmer_analysis_v2_amd as pkg
from depth_model import rec, records
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu

K = 21
PAD = 64  # canary bytes in front of and behind an array
_SRC = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "kc_depth.hpp")).read()
T = int(re.search(r"DEPTH_TPB = (\d+);", _SRC).group(1)) * int(re.search(r"DEPTH_ITEMS = (\d+);", _SRC).group(1))  # the scan's tile
NONE_REC = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, D.KIND_NONE, (0, 0))


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def lengths_index(lens, seed=1, **kw):
    """a counter with an index over random contigs of these lengths"""
    rng = np.random.default_rng(seed)
    text = rand_seq(rng, sum(lens))
    contigs, at = [], 0
    for n in lens:
        contigs.append(text[at:at + n])
        at += n
    block, offsets = A.join_block(contigs)
    kc = pkg.KmerCounter(K, **kw)
    kc.index_contigs(np.frombuffer(block.encode(), dtype=np.uint8).copy(), np.array(offsets, dtype=np.uint64))
    assert kc.contig_index_info() == (sum(lens) + len(lens), len(lens))
    return kc


def stats_dict(st):
    return {n: int(getattr(st, n)) for n, _ in st._fields_}


UNTOUCHED = dict(dict.fromkeys(D.DEPTH_STATS, 0), records=99)


def device_depths(kc, lens, alns, min_score=0, min_len=0, edge_clip=0, flags=0, nreads=0, expect=0, shift=0, want_depths=True, want_ctgs=True,
                  want_stats=True):
    """the call on device arrays of exactly the needed size inside canaries: (depths, ctgs, stats).  expect != 0: the
    status is checked, and that nothing at all was written; shift: bytes by which the record arrays are misaligned."""
    import torch
    nbytes, n_ctgs, na = sum(lens) + len(lens), len(lens), len(alns)
    h_in = np.full(na * 32 + 2 * PAD + 16, 0xCD, dtype=np.uint8)
    h_in[PAD + shift:PAD + shift + na * 32] = np.frombuffer(alns.tobytes(), dtype=np.uint8)
    d_in = torch.from_numpy(h_in).cuda()
    d_dep = torch.full((nbytes * 2 + 2 * PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    d_ctg = torch.full((n_ctgs * 32 + 2 * PAD + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = _lib.kc_depth_stats(records=99)
    rc = pkg.lib().kc_aln_depths(kc._h, d_in.data_ptr() + PAD + shift, na, nreads, 1, min_score, min_len, edge_clip, flags,
                                 d_dep.data_ptr() + PAD if want_depths else None, d_ctg.data_ptr() + PAD + shift if want_ctgs else None,
                                 C.byref(st) if want_stats else None)
    h_dep, h_ctg = d_dep.cpu().numpy(), d_ctg.cpu().numpy()
    assert (d_in.cpu().numpy() == h_in).all(), "the input records were written"
    if expect:
        assert rc == expect
        assert (h_dep == 0xAB).all() and (h_ctg == 0xAB).all(), "a refused call wrote"
        assert stats_dict(st) == UNTOUCHED, "a refused call wrote statistics"
        return rc
    assert rc == 0, pkg.lib().kc_last_error()
    assert (h_dep[:PAD] == 0xAB).all() and (h_dep[PAD + nbytes * 2:] == 0xAB).all(), "a canary was written"
    assert (h_ctg[:PAD + shift] == 0xAB).all() and (h_ctg[PAD + shift + n_ctgs * 32:] == 0xAB).all(), "a canary was written"
    if not want_depths:
        assert (h_dep == 0xAB).all()
    if not want_ctgs:
        assert (h_ctg == 0xAB).all()
    if not want_stats:
        assert stats_dict(st) == UNTOUCHED
    return (h_dep[PAD:PAD + nbytes * 2].copy().view(np.uint16), h_ctg[PAD + shift:PAD + shift + n_ctgs * 32].copy().view(D.CTG_DEPTH_DTYPE),
            stats_dict(st))


def compare(kc, lens, alns, **kw):
    want = D.aln_depths(lens, alns, **kw)
    got = device_depths(kc, lens, alns, **kw)
    assert got[2] == want[2]
    if got[1].tobytes() != want[1].tobytes():
        diff = [u for u in range(len(lens)) if got[1][u].tobytes() != want[1][u].tobytes()]
        assert not diff, (diff[:5], got[1][diff[:5]], want[1][diff[:5]])
    if got[0].tobytes() != want[0].tobytes():
        diff = np.nonzero(got[0] != want[0])[0]
        assert not len(diff), (diff[:8], got[0][diff[:8]], want[0][diff[:8]])
    return want


def random_records(rng, lens, n, max_len=150, nreads=None):
    rows = []
    live = [u for u, x in enumerate(lens) if x > 0]
    for i in range(n):
        u = live[int(rng.integers(0, len(live)))]
        span = int(rng.integers(1, min(max_len, lens[u]) + 1))
        a = [0, lens[u] - span, int(rng.integers(0, lens[u] - span + 1))][int(rng.integers(0, 3))]
        rows.append(rec(i if nreads is None else int(rng.integers(0, nreads)), u, a, a + span, score=int(rng.integers(1, 300)), orient=i & 1,
                        kind=int(rng.integers(0, 2))))
    return records(rows)


# ---- the scan's tiles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [T - 1, T, T + 1, 3 * T + 1])
def test_blocks_around_the_tile_size(nbytes):
    rng = np.random.default_rng(nbytes)
    # one long contig and a few short ones; the separators take len(lens) bytes
    lens = [nbytes - 40 - 57 - 4, 40, 57, 0]
    assert sum(lens) + len(lens) == nbytes
    alns = random_records(rng, lens, 300)
    with lengths_index(lens) as kc:
        compare(kc, lens, alns)
        compare(kc, lens, alns, edge_clip=5, flags=D.PER_CONTIG)
    lens = [nbytes - 1]  # one contig: its separator is the block's last byte
    with lengths_index(lens) as kc:
        compare(kc, lens, np.concatenate([random_records(rng, lens, 200), records([rec(0, 0, 0, nbytes - 1), rec(0, 0, nbytes - 2, nbytes - 1)])]))


def test_records_at_tile_and_contig_boundaries():
    lens = [T + 500, T - 502, 700]  # contig 1's separator is byte 2T - 1, a tile's last; contig 2 starts on the next tile's first
    o = D.block_offsets(lens)
    assert o[2] == 2 * T
    rows = [rec(0, 0, T - 50, T),          # ends on the first tile's last byte
            rec(1, 0, T, T + 60),          # starts on the second tile's first
            rec(2, 0, T - 1, T + 1),       # straddles
            rec(3, 1, lens[1] - 80, lens[1]),  # ends at the contig's end, right in front of the separator
            rec(4, 2, 0, 90),              # the next contig starts covered, on a tile's first byte
            rec(5, 0, lens[0] - 1, lens[0]), rec(6, 1, 0, 1), rec(7, 0, 0, lens[0])]
    with lengths_index(lens) as kc:
        out, ctgs, st = compare(kc, lens, records(rows))
        assert int(out[o[1] + lens[1] - 1]) == 1 and int(out[o[2] - 1]) == 0 and int(out[o[2]]) == 1
        assert int(out[T - 1]) == 3 and int(out[T]) == 3
        for e in (1, 49, 50):
            compare(kc, lens, records(rows), edge_clip=e)


def test_contig_lengths_from_nothing_to_a_wave_and_over():
    lens = [0, 1, 0, 0, 63, 64, 65, 0, 7, 8, 9, 511, 512, 513, 1, 0]
    rng = np.random.default_rng(5)
    alns = np.concatenate([random_records(rng, lens, 500, max_len=600), records([rec(0, 1, 0, 1)] * 3 + [rec(0, u, 0, lens[u]) for u in (4, 5, 6, 14)])])
    with lengths_index(lens) as kc:
        out, ctgs, st = compare(kc, lens, alns)
        assert [int(x) for x in ctgs["len"]] == lens and int(ctgs[1]["min_depth"]) >= 3 and int(ctgs[0]["alns"]) == 0
        compare(kc, lens, alns, flags=D.PER_CONTIG)
        compare(kc, lens, records([]))
    lens = [0] * 300  # separators only: more contigs than bytes a thread holds
    with lengths_index(lens) as kc:
        out, ctgs, st = compare(kc, lens, records([NONE_REC]))
        assert st["none"] == 1 and not ctgs.view(np.uint8).any()


def test_many_short_contigs_beside_a_long_one():
    rng = np.random.default_rng(6)
    lens = [int(x) for x in rng.integers(25, 61, size=5000)]
    lens.insert(2500, 300020)
    alns = random_records(rng, lens, 12000)
    with lengths_index(lens) as kc:
        out, ctgs, st = compare(kc, lens, alns, edge_clip=2)
        assert st["used"] > 8000 and int(ctgs[2500]["alns"]) > 0 and int(ctgs["covered"].astype(np.int64).sum()) == st["bases_covered"]
        compare(kc, lens, alns, flags=D.PER_CONTIG)


@pytest.mark.parametrize("n", [65535, 65536, 70000])
def test_saturation(n):
    lens = [30, 2 * T, 10]
    alns = np.concatenate([records([rec(0, 1, T - 3, T + 4)] * n), records([rec(0, 1, 0, T - 3), rec(1, 2, 0, 10)])])
    with lengths_index(lens) as kc:
        out, ctgs, st = compare(kc, lens, alns)
        assert st["saturated"] == (7 if n > 65535 else 0) and int(ctgs[1]["max_depth"]) == n  # the interval straddles two tiles
        assert int(out[31 + T]) == 65535 and int(out[31 + T - 4]) == 1 and int(out[31 + T + 4]) == 0
    with lengths_index([9]) as kc:  # the mean is capped like a depth
        out, ctgs, st = compare(kc, [9], records([rec(0, 0, 0, 9)] * n), flags=D.PER_CONTIG)
        assert int(ctgs[0]["mean"]) == min(n, 65535) == int(out[5]) and int(ctgs[0]["min_depth"]) == n and int(out[9]) == 0


# ---- the definition's corners -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [0, 1, K, 1024])
def test_edge_clip(e):
    lens = [5000, 40]
    rows = []
    for span in (1, 2, 2 * e, 2 * e + 1, 150, 2500):
        if span == 0:
            continue
        for a in (0, 1, e, e + 1, 2000, lens[0] - span - e - 1, lens[0] - span - 1, lens[0] - span):
            if 0 <= a and a + span <= lens[0]:
                rows.append(rec(len(rows), 0, a, a + span))
    rows += [rec(0, 1, 0, 40), rec(0, 1, 1, 40), rec(0, 1, 0, 39), rec(0, 1, 1, 39), rec(0, 0, 0, 5000)]
    with lengths_index(lens) as kc:
        out, ctgs, st = compare(kc, lens, records(rows), edge_clip=e)
        assert st["clipped_away"] + st["used"] == len(rows) and (e == 0) == (st["clipped_away"] == 0)


def test_filter_thresholds_and_none_records():
    lens = [400]
    rows = [rec(0, 0, 10, 110, score=200), rec(1, 0, 10, 109, score=200), rec(2, 0, 10, 111, score=200), rec(3, 0, 10, 110, score=199),
            rec(4, 0, 10, 110, score=201), rec(5, 0, 0, 400, score=0xFFFFFFFF), NONE_REC, (9, 0, 0, 0, 0, 0, 0, 0, 0, 1, D.KIND_NONE, (0, 0))]
    with lengths_index(lens) as kc:
        out, ctgs, st = compare(kc, lens, records(rows), min_score=200, min_len=100)
        assert (st["none"], st["filtered"], st["used"]) == (2, 2, 4)
        compare(kc, lens, records(rows), min_score=201, min_len=101)
        compare(kc, lens, records(rows), min_score=0xFFFFFFFF)
        compare(kc, lens, records(rows), min_len=0xFFFFFFFF)
        compare(kc, lens, records([NONE_REC] * 5))


def test_best_only():
    rng = np.random.default_rng(8)
    lens = [3000, 50, 0, 2000]
    nreads = 700
    alns = random_records(rng, lens, 4000, nreads=nreads)
    alns["score"][::3] = 77  # many equal scores within a read
    with lengths_index(lens) as kc:
        out, ctgs, st = compare(kc, lens, alns, flags=D.BEST_ONLY, nreads=nreads)
        assert st["not_best"] > 2000 and st["used"] > 500
        out2, _, _ = compare(kc, lens, alns[rng.permutation(len(alns))], flags=D.BEST_ONLY, nreads=nreads, min_score=50, edge_clip=3)
        compare(kc, lens, alns, flags=D.BEST_ONLY | D.PER_CONTIG, nreads=nreads)
        # the read field is part of validity only with the flag
        stray = records([rec(nreads, 0, 0, 10)])
        compare(kc, lens, stray)
        device_depths(kc, lens, stray, flags=D.BEST_ONLY, nreads=nreads, expect=_lib.KC_ERR_INVALID_ARG)
        compare(kc, lens, stray, flags=D.BEST_ONLY, nreads=nreads + 1)


# ---- the protocol -------------------------------------------------------------------------------------------------------
def small_case():
    lens = [300, 0, 250]
    alns = records([rec(0, 0, 10, 160, score=300), rec(1, 2, 50, 199, score=280, orient=1, kind=1), rec(1, 2, 51, 200, score=120, kind=1),
                    rec(2, 0, 200, 300, score=190), NONE_REC])
    return lens, alns


def test_null_outputs_no_records_host_and_wrapper():
    import torch
    lens, alns = small_case()
    with lengths_index(lens, time_kernels=True) as kc:
        kc.kernel_times(clear=True)
        want = compare(kc, lens, alns)
        times = {n: v[0] for n, v in kc.kernel_times(clear=True).items()}
        assert times == {"kc_depth_check_kernel": 1, "kc_depth_mark_kernel": 1, "kc_depth_tile_sums_kernel": 1, "kc_depth_scan_kernel": 1,
                         "kc_depth_rescan_kernel": 1, "kc_depth_ctg_kernel": 1}
        compare(kc, lens, alns, flags=D.BEST_ONLY | D.PER_CONTIG, nreads=3)
        times = {n: v[0] for n, v in kc.kernel_times(clear=True).items()}
        assert times == {"kc_depth_check_kernel": 1, "kc_depth_best_kernel": 1, "kc_depth_mark_kernel": 1, "kc_depth_tile_sums_kernel": 1,
                         "kc_depth_scan_kernel": 1, "kc_depth_rescan_kernel": 1, "kc_depth_ctg_kernel": 1, "kc_depth_fill_kernel": 1}
        for flags in (0, D.PER_CONTIG):
            w = D.aln_depths(lens, alns, flags=flags)
            for off in ("want_depths", "want_ctgs", "want_stats"):
                got = device_depths(kc, lens, alns, flags=flags, **{off: False})
                if off != "want_depths":
                    assert got[0].tobytes() == w[0].tobytes()
                if off != "want_ctgs":
                    assert got[1].tobytes() == w[1].tobytes()
                if off != "want_stats":
                    assert got[2] == w[2]
            got = device_depths(kc, lens, alns, flags=flags, want_depths=False, want_ctgs=False)
            assert got[2] == w[2]
        # no records: zeros, written
        out, ctgs, st = compare(kc, lens, records([]))
        assert not out.any() and st == dict.fromkeys(D.DEPTH_STATS, 0) and [int(x) for x in ctgs["len"]] == lens
        # host arrays, inside canaries of their own
        nbytes = sum(lens) + len(lens)
        h_dep = np.full(nbytes + 2, 0xABAB, dtype=np.uint16)
        h_ctg = np.full((len(lens) + 2) * 32, 0xAB, dtype=np.uint8)
        st = _lib.kc_depth_stats()
        rc = pkg.lib().kc_aln_depths(kc._h, alns.ctypes.data, len(alns), 0, 0, 0, 0, 0, 0, h_dep.ctypes.data + 2, h_ctg.ctypes.data + 32, C.byref(st))
        assert rc == 0 and stats_dict(st) == want[2]
        assert h_dep[1:-1].tobytes() == want[0].tobytes() and h_ctg[32:-32].tobytes() == want[1].tobytes()
        assert h_dep[0] == h_dep[-1] == 0xABAB and (h_ctg[:32] == 0xAB).all() and (h_ctg[-32:] == 0xAB).all()
        # the wrapper, both modes
        d, c, s = kc.aln_depths(alns)
        assert d.dtype == np.uint16 and c.dtype == D.CTG_DEPTH_DTYPE and (d.tobytes(), c.tobytes(), s) == (want[0].tobytes(), want[1].tobytes(), want[2])
        w = D.aln_depths(lens, alns, 150, 100, 4, D.BEST_ONLY | D.PER_CONTIG, 3)
        d_alns = torch.from_numpy(np.frombuffer(alns.tobytes(), dtype=np.uint8).copy()).cuda()
        d, c, s = kc.aln_depths(d_alns, min_score=150, min_len=100, edge_clip=4, best_only=True, per_contig=True, nreads=3)
        assert d.is_cuda and c.is_cuda and d.cpu().numpy().view(np.uint16).tobytes() == w[0].tobytes()
        assert c.cpu().numpy().tobytes() == w[1].tobytes() and s == w[2]
        # device record arrays are 16-byte aligned; the ranges, with a context this time
        assert device_depths(kc, lens, alns, shift=8, expect=_lib.KC_ERR_INVALID_ARG) == _lib.KC_ERR_INVALID_ARG
        assert b"16-byte aligned" in pkg.lib().kc_last_error()
        device_depths(kc, lens, alns, edge_clip=1025, expect=_lib.KC_ERR_INVALID_ARG)
        device_depths(kc, lens, alns, flags=4, expect=_lib.KC_ERR_INVALID_ARG)
        compare(kc, lens, alns)


def test_names_and_launch_counts_in_the_kernel_times():
    lens, alns = small_case()
    with lengths_index(lens, time_kernels=True) as kc:
        kc.kernel_times(clear=True)
        kc.aln_depths(alns, best_only=True, per_contig=True, nreads=3)  # every optional kernel runs
        t = kc.kernel_times()
    want = {"kc_depth_check_kernel": 1, "kc_depth_best_kernel": 1, "kc_depth_mark_kernel": 1, "kc_depth_tile_sums_kernel": 1,
            "kc_depth_scan_kernel": 1, "kc_depth_rescan_kernel": 1, "kc_depth_ctg_kernel": 1, "kc_depth_fill_kernel": 1}
    assert {n: c for n, (c, _) in t.items()} == want


def test_invalid_records_are_named_and_nothing_is_written():
    lens, alns = small_case()
    good = alns[3]  # contig 0 (300 bases): cstart 200, cstop 300, rstart 0, rstop 100

    def forged(**kw):
        r = good.copy()
        for k, v in kw.items():
            r[k] = v
        return r

    none = records([NONE_REC])[0]
    bad = [forged(ctg=3), forged(ctg=0xFFFFFFFF), forged(orient=2), forged(orient=255), forged(kind=3), forged(kind=255), forged(cstop=301),
           forged(cstart=300), forged(cstart=301, cstop=300), forged(cstop=200), forged(rstart=100), forged(rstart=101), forged(rstop=1025, rstart=900),
           forged(rstop=0, rstart=0), forged(ctg=1, cstart=0, cstop=1), forged(ctg=3, kind=2)]
    none["ctg"], none["orient"] = 2, 1
    ok = [forged(rstop=1024), forged(cstart=299), forged(kind=2, cstart=9, cstop=3, rstart=9, rstop=2), none, forged(read=0xFFFFFFFF)]
    with lengths_index(lens) as kc:
        L = pkg.lib()
        compare(kc, lens, records(ok))
        for b in bad:
            with pytest.raises(D.BadRecord):
                D.aln_depths(lens, records([b]))
            assert device_depths(kc, lens, records([b]), expect=_lib.KC_ERR_INVALID_ARG)
            assert b"kc_aln_depths: record 0 " in L.kc_last_error()
            many = np.concatenate([alns, alns[:3], records([b]), alns, records([b]), alns])
            with pytest.raises(D.BadRecord) as e:
                D.aln_depths(lens, many)
            assert e.value.index == 8
            device_depths(kc, lens, many, expect=_lib.KC_ERR_INVALID_ARG)
            assert b"record 8 " in L.kc_last_error()
        compare(kc, lens, alns)


def test_state_rebuilt_index_and_ranks():
    lens, alns = small_case()
    with pkg.KmerCounter(K) as kc:
        assert device_depths(kc, lens, alns, expect=_lib.KC_ERR_STATE) == _lib.KC_ERR_STATE  # no index
        assert pkg.lib().kc_ctg_index_info(kc._h, None, None) == _lib.KC_ERR_STATE
    with lengths_index(lens) as kc:
        want = compare(kc, lens, alns)
        kc.clear_contig_index()
        device_depths(kc, lens, alns, expect=_lib.KC_ERR_STATE)
        with pytest.raises(pkg.KcError):
            kc.contig_index_info()
    with lengths_index(lens) as kc:
        kc.reset()
        device_depths(kc, lens, alns, expect=_lib.KC_ERR_STATE)
    # a rebuilt index with other lengths: other arrays, and the old records do not fit
    lens2 = [250, 301, 7]
    with lengths_index(lens) as kc:
        rng = np.random.default_rng(3)
        block, offsets = A.join_block([rand_seq(rng, n) for n in lens2])
        kc.index_contigs(np.frombuffer(block.encode(), dtype=np.uint8).copy(), np.array(offsets, dtype=np.uint64))
        assert kc.contig_index_info() == (sum(lens2) + 3, 3)
        device_depths(kc, lens2, alns, expect=_lib.KC_ERR_INVALID_ARG)
        alns2 = alns.copy()
        alns2["ctg"] = [1, 0, 0, 1, 0]
        got = compare(kc, lens2, alns2)
        assert int(got[1][1]["depth_sum"]) == int(want[1][0]["depth_sum"])
    with lengths_index(lens, rank_me=1, rank_n=2) as kc:
        compare(kc, lens, alns)


def test_the_whole_chain_feeds_the_contig_pass():
    """count -> index_unitigs -> align_reads -> align_gapped -> aln_depths(per_contig) -> submit_ctg_block on a second
    counter -> finalize, against the oracle fed the same depths; the first counter answers as before afterwards."""
    import torch
    from gap_model import _plant
    from oracle import cpu_oracle as O
    from test_gpu_parity import assert_same
    from test_gpu_gap_align import read_arrays, revc
    rng = np.random.default_rng(64)
    chains = [rand_seq(rng, m) for m in (700, 400, 1000)]
    cover = []
    for seq in chains:
        for a in range(0, len(seq) - K, 100):
            cover += [seq[a:a + 200]] * 2
    b, o = read_arrays(cover)
    q = np.full(len(b), ord("I"), dtype=np.uint8)
    queries = []
    for i in range(200):
        seq = chains[i % 3]
        a = int(rng.integers(1, len(seq) - 154))
        rp = _plant(rng, seq[a:a + 150], i % 3, i % 2)[:150]
        queries.append(rp if i % 2 else revc(rp))
    qb, qo = read_arrays(queries)
    with pkg.KmerCounter(K) as kc:
        kc.submit_reads(b, q, o)
        kc.finalize()
        strings = kc.unitig_strings()
        contigs = [s for s, _ in strings]
        lens = [len(s) for s in contigs]
        keys, counts, left, right = [np.array(x) for x in kc.sorted_results()]
        looked = [np.array(x) for x in kc.lookup(keys)]
        kc.index_unitigs()
        d_qb, d_qo = torch.from_numpy(qb).cuda(), torch.from_numpy(qo.view(np.int64)).cuda()
        alns, _, a_st = kc.align_reads(d_qb, d_qo)
        gaps, g_st = kc.align_gapped(d_qb, d_qo, alns)
        depths, ctgs, st = kc.aln_depths(gaps, min_score=100, edge_clip=2, best_only=True, per_contig=True, nreads=len(queries))
        h_gaps = gaps.cpu().numpy().view(D.GAP_ALN_DTYPE)
        want = D.aln_depths(lens, h_gaps, min_score=100, edge_clip=2, flags=D.BEST_ONLY | D.PER_CONTIG, nreads=len(queries))
        h_depths = depths.cpu().numpy().view(np.uint16)
        assert h_depths.tobytes() == want[0].tobytes() and ctgs.cpu().numpy().tobytes() == want[1].tobytes() and st == want[2]
        assert st["used"] > 120 and len(set(int(x) for x in want[1]["mean"])) > 1
        seqs, _, offsets, _, _ = kc._unitigs(False, False)
        with pkg.KmerCounter(K) as kc2:
            kc2.submit_reads(b, q, o)
            kc2.begin_ctg_kmers(sum(lens))
            kc2.submit_ctg_block(seqs, depths)
            kc2.finalize()
            got = [np.array(x) for x in kc2.sorted_results()]
        offs = D.block_offsets(lens)
        ctg_depths = [int(h_depths[offs[u]]) if lens[u] else 0 for u in range(len(lens))]
        orc = O.Oracle(K, nranks=1, nthreads=1)
        orc.add_reads(b, q, o)
        for u in range(len(lens)):
            orc.add_ctg(contigs[u], ctg_depths[u])
        assert_same(got, orc.finalize())
        orc.close()
        # nothing else has changed
        again, _, again_st = kc.align_reads(d_qb, d_qo)
        assert again.cpu().numpy().tobytes() == alns.cpu().numpy().tobytes() and again_st == a_st
        g2, g2_st = kc.align_gapped(d_qb, d_qo, alns)
        assert g2.cpu().numpy().tobytes() == h_gaps.tobytes() and g2_st == g_st
        for x, y in zip((keys, counts, left, right), [np.array(x) for x in kc.sorted_results()]):
            assert (x == y).all()
        for x, y in zip(looked, [np.array(x) for x in kc.lookup(keys)]):
            assert (x == y).all()
        assert kc.unitig_strings() == strings
