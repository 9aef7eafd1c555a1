"""kc_pair_inserts (csrc/kc_depth.hpp) against the host model tests/depth_model.py, byte for byte: the histogram, the
pairs' records and the statistics on the same inputs.  The model is never replaced by a second device run.

Fragments of known length f are cut from a contig at known places: mate 1 = frag[:L], mate 2 = revcomp(frag[-L:]), run
through align_reads -> align_gapped, so that insert == f by construction, not only by the model.  The call needs the
reads' offsets only, so the protocol cases forge records and offsets.  Every device call goes through device_pairs:
all arrays of exactly their size inside canaries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import depth_model as D
import mhm2_kmer_analysis_v2_amd as pkg
from depth_model import rec, records
from mhm2_kmer_analysis_v2_amd import _lib
from test_gpu_aln_depths import K, NONE_REC, PAD, lengths_index, rand_seq
from test_gpu_gap_align import block_arrays, read_arrays, revc

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "kc_depth.hpp")).read()
LDS_BINS = int(re.search(r"PAIR_LDS_BINS = (\d+);", _SRC).group(1))  # max_insert + 1 bins fit in LDS up to here
L = 100
STAT_FIELDS = ("pairs", "cls", "insert_sum", "insert_sq_sum", "reads_with_best")


def stats_dict(st):
    return {"pairs": int(st.pairs), "cls": [int(x) for x in st.cls], "insert_sum": int(st.insert_sum), "insert_sq_sum": int(st.insert_sq_sum),
            "reads_with_best": int(st.reads_with_best)}


UNTOUCHED = {"pairs": 99, "cls": [0] * 7, "insert_sum": 0, "insert_sq_sum": 0, "reads_with_best": 0}


def offsets_of(read_lens):
    offs = np.zeros(len(read_lens) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(read_lens)
    return offs


def device_pairs(kc, read_lens, alns, max_insert=1000, min_score=0, min_len=0, expect=0, shift=0, want_hist=True, want_pairs=True, want_stats=True):
    """the call on device arrays of exactly the needed size inside canaries: (hist, pairs, stats).  expect != 0: the
    status is checked, and that nothing at all was written; shift: bytes by which the record arrays are misaligned."""
    import torch
    nreads, na, nb = len(read_lens), len(alns), min(max_insert, 65535) + 1
    h_in = np.full(na * 32 + 2 * PAD + 16, 0xCD, dtype=np.uint8)
    h_in[PAD + shift:PAD + shift + na * 32] = np.frombuffer(alns.tobytes(), dtype=np.uint8)
    d_in = torch.from_numpy(h_in).cuda()
    d_o = torch.from_numpy(offsets_of(read_lens).view(np.int64)).cuda()
    d_hist = torch.full((nb * 8 + 2 * PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    d_pairs = torch.full((nreads // 2 * 16 + 2 * PAD + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = _lib.kc_insert_stats(pairs=99)
    rc = pkg.lib().kc_pair_inserts(kc._h, d_o.data_ptr(), nreads, d_in.data_ptr() + PAD + shift, na, 1, min_score, min_len, max_insert,
                                   d_hist.data_ptr() + PAD if want_hist else None, d_pairs.data_ptr() + PAD + shift if want_pairs else None,
                                   C.byref(st) if want_stats else None)
    h_hist, h_pairs = d_hist.cpu().numpy(), d_pairs.cpu().numpy()
    assert (d_in.cpu().numpy() == h_in).all(), "the input records were written"
    if expect:
        assert rc == expect
        assert (h_hist == 0xAB).all() and (h_pairs == 0xAB).all(), "a refused call wrote"
        assert stats_dict(st) == UNTOUCHED, "a refused call wrote statistics"
        return rc
    assert rc == 0, pkg.lib().kc_last_error()
    np_ = nreads // 2
    assert (h_hist[:PAD] == 0xAB).all() and (h_hist[PAD + nb * 8:] == 0xAB).all(), "a canary was written"
    assert (h_pairs[:PAD + shift] == 0xAB).all() and (h_pairs[PAD + shift + np_ * 16:] == 0xAB).all(), "a canary was written"
    if not want_hist:
        assert (h_hist == 0xAB).all()
    if not want_pairs:
        assert (h_pairs == 0xAB).all()
    if not want_stats:
        assert stats_dict(st) == UNTOUCHED
    return (h_hist[PAD:PAD + nb * 8].copy().view(np.uint64), h_pairs[PAD + shift:PAD + shift + np_ * 16].copy().view(D.PAIR_DTYPE), stats_dict(st))


def compare(kc, ctg_lens, read_lens, alns, max_insert=1000, **kw):
    want = D.pair_inserts(ctg_lens, read_lens, alns, max_insert, **kw)
    got = device_pairs(kc, read_lens, alns, max_insert, **kw)
    assert got[2] == want[2]
    if got[1].tobytes() != want[1].tobytes():
        diff = [p for p in range(len(want[1])) if got[1][p].tobytes() != want[1][p].tobytes()]
        assert not diff, (diff[:5], got[1][diff[:5]], want[1][diff[:5]])
    assert (got[0] == want[0]).all(), np.nonzero(got[0] != want[0])[0][:8]
    return want


def mates(frag, flip=False):
    m1, m2 = frag[:L], revc(frag[-L:])
    return [m2, m1] if flip else [m1, m2]


def aligned(kc, reads):
    """the reads' gapped records, through the device's own two alignment steps (host arrays)"""
    b, o = read_arrays(reads)
    alns, _, _ = kc.align_reads(b, o)
    gaps, _ = kc.align_gapped(b, o, alns)
    return gaps


def indexed(contigs, **kw):
    kc = pkg.KmerCounter(K, **kw)
    kc.index_contigs(*block_arrays(contigs))
    return kc


# ---- by construction ----------------------------------------------------------------------------------------------------
def test_pairs_of_known_fragments():
    rng = np.random.default_rng(70)
    contigs = [rand_seq(rng, 4000), rand_seq(rng, 900)]
    c0, c1 = contigs
    M = 1000  # max_insert
    P, TL = D.PAIR_PROPER, D.PAIR_TOO_LONG
    cases = []  # (reads of the pair, class, insert)
    for f, cls in ((L, P), (L + 1, P), (M, P), (M + 1, TL)):
        for flip in (False, True):
            a = int(rng.integers(0, len(c0) - f))
            cases.append((mates(c0[a:a + f], flip), cls, f))
    # an insertion in mate 1, a deletion in mate 2: the fragment on the contig is what counts
    frag = c0[500:900]
    m1, m2 = mates(frag)
    cases.append(([m1[:50] + "AC" + m1[50:98], m2], P, 400))  # mate 1 ends two contig bases early; only where it begins counts
    frag = c0[1500:1902]
    rp2 = frag[-102:-52] + frag[-50:]  # R' of mate 2: 100 bases over 102 of the contig
    cases.append(([frag[:L], revc(rp2)], P, 402))
    # mates hanging over the contig's ends: soft-clipped, projected
    junk = rand_seq(rng, 30)
    cases.append((mates(junk + c0[:370]), P, 400))
    cases.append((mates(c0[-370:] + junk), P, 400))
    cases.append((mates(junk + c1 + junk[::-1], flip=True), P, len(c1) + 60))
    # everted, same orientation, two contigs, one mate or both without a record
    cases.append(([c0[2000:2000 + L], revc(c0[1500:1500 + L])], D.PAIR_EVERTED, 0))
    cases.append(([c0[2000:2000 + L], revc(c0[1999:1999 + L])], D.PAIR_EVERTED, 0))
    cases.append(([c0[2000:2000 + L], c0[2300:2300 + L]], D.PAIR_SAME_ORIENT, 0))
    cases.append(([revc(c0[2000:2000 + L]), revc(c0[2300:2300 + L])], D.PAIR_SAME_ORIENT, 0))
    cases.append(([c0[100:100 + L], revc(c1[300:300 + L])], D.PAIR_DIFF_CTG, 0))
    cases.append(([c0[100:100 + L], rand_seq(rng, L)], D.PAIR_ONE, 0))
    cases.append(([rand_seq(rng, L), revc(c0[100:100 + L])], D.PAIR_ONE, 0))
    cases.append(([rand_seq(rng, L), rand_seq(rng, 40)], D.PAIR_NONE, 0))
    cases.append((["", ""], D.PAIR_NONE, 0))
    reads = [r for c in cases for r in c[0]]
    read_lens = [len(r) for r in reads]
    ctg_lens = [len(c) for c in contigs]
    with indexed(contigs) as kc:
        gaps = aligned(kc, reads)
        hist, pairs, st = compare(kc, ctg_lens, read_lens, gaps, M)
        assert [(int(p["cls"]), int(p["insert"])) for p in pairs] == [(c[1], c[2]) for c in cases]
        proper = [c[2] for c in cases if c[1] == P]
        assert st["cls"][P] == len(proper) and st["insert_sum"] == sum(proper) and (hist == np.bincount(proper, minlength=M + 1)).all()
        # a mate with two records of equal score: the lower index wins, wherever the other one points
        twin = gaps[int(pairs[0]["aln0"])].copy()  # the forward mate of a fragment of L bases
        shift = 700 if int(twin["cstop"]) + 700 <= len(c0) else -700
        twin["cstart"] += shift
        twin["cstop"] += shift
        both = np.concatenate([gaps, records([twin])])
        w = compare(kc, ctg_lens, read_lens, both, M)
        assert w[1].tobytes() == pairs.tobytes()
        first = np.concatenate([records([twin]), gaps])
        w = compare(kc, ctg_lens, read_lens, first, M)
        assert int(w[1][0]["aln0"]) == 0 and int(w[1][1]["aln0"]) == int(pairs[1]["aln0"]) + 1
        assert (int(w[1][0]["cls"]), int(w[1][0]["insert"])) == ((D.PAIR_EVERTED, 0) if shift > 0 else (P, L + 700))
        # any order of the records: the same pairs up to the indices
        perm = rng.permutation(len(gaps))
        w = compare(kc, ctg_lens, read_lens, gaps[perm], M)
        assert (w[1]["cls"] == pairs["cls"]).all() and (w[1]["insert"] == pairs["insert"]).all() and (w[0] == hist).all()
        # the bins in LDS, at the largest size that fits and the first that does not, and at the limit
        for m in (1, L, LDS_BINS - 1, LDS_BINS, 65535):
            w = compare(kc, ctg_lens, read_lens, gaps, m)
            assert w[2]["cls"][P] == sum(1 for f in proper if f <= m) + (1 if m >= M + 1 else 0) * 2
        compare(kc, ctg_lens, read_lens, gaps, M, min_score=199)
        compare(kc, ctg_lens, read_lens, gaps, M, min_score=200, min_len=L)
        compare(kc, ctg_lens, read_lens, gaps, M, min_len=L + 1)


@pytest.mark.parametrize("max_insert", [1000, 65535])
def test_twenty_thousand_pairs_of_drawn_lengths(max_insert):
    rng = np.random.default_rng(71)
    ctg = rand_seq(rng, 60000)
    n = 20000
    f = np.clip(rng.normal(420, 60, size=n).round().astype(np.int64), L, 1200)
    at = rng.integers(0, len(ctg) - f)
    flip = rng.integers(0, 2, size=n)
    reads = []
    for i in range(n):
        reads += mates(ctg[int(at[i]):int(at[i]) + int(f[i])], bool(flip[i]))
    with indexed([ctg]) as kc:
        gaps = aligned(kc, reads)
        hist, pairs, st = compare(kc, [len(ctg)], [L] * (2 * n), gaps, max_insert)
        proper = pairs["cls"] == D.PAIR_PROPER
        assert proper.sum() > n * 0.97  # a read whose every seed is repeated in a random contig is rare
        assert (hist == np.bincount(f[proper], minlength=max_insert + 1).astype(np.uint64)).all()
        assert (pairs["insert"][proper] == f[proper]).all() and st["insert_sum"] == int(f[proper].sum())
        assert max_insert < 1200 or (proper | (pairs["cls"] <= D.PAIR_ONE)).all()
        # the wrapper's floats are the integers' arithmetic
        b, o = read_arrays(reads)
        h2, p2, s2 = kc.pair_inserts(o, gaps, max_insert=max_insert)
        assert h2.tobytes() == hist.tobytes() and p2.tobytes() == pairs.tobytes() and {k: s2[k] for k in STAT_FIELDS} == st
        assert abs(s2["mean"] - f[proper].mean()) < 1e-6 and abs(s2["stddev"] - f[proper].std()) < 1e-6


# ---- the protocol -------------------------------------------------------------------------------------------------------
def small_case():
    ctg_lens = [300, 0, 250]
    read_lens = [150, 150, 100, 120, 0, 90]
    alns = records([rec(0, 0, 10, 160, score=300), rec(1, 0, 100, 250, score=280, orient=1, kind=1), rec(1, 2, 51, 200, rstop=150, score=120, kind=1),
                    rec(2, 0, 200, 300, score=190), rec(3, 0, 5, 105, rstart=20, score=190, orient=1), NONE_REC, rec(5, 2, 0, 90, orient=1)])
    return ctg_lens, read_lens, alns


def test_null_outputs_no_records_host_and_wrapper():
    import torch
    ctg_lens, read_lens, alns = small_case()
    with lengths_index(ctg_lens, time_kernels=True) as kc:
        kc.kernel_times(clear=True)
        want = compare(kc, ctg_lens, read_lens, alns)
        assert [int(x) for x in want[1]["cls"]] == [D.PAIR_PROPER, D.PAIR_EVERTED, D.PAIR_ONE] and int(want[1][0]["insert"]) == 240
        times = {n: v[0] for n, v in kc.kernel_times(clear=True).items()}
        assert times == {"kc_align_lengths_kernel<pair>": 1, "kc_depth_check_kernel<pair>": 1, "kc_depth_best_kernel<pair>": 1,
                         "kc_pair_classify_kernel<lds>": 1}
        compare(kc, ctg_lens, read_lens, alns, LDS_BINS)
        assert {n: v[0] for n, v in kc.kernel_times(clear=True).items()}["kc_pair_classify_kernel"] == 1
        for m in (1000, 65535):
            for off in ("want_hist", "want_pairs", "want_stats"):
                w = D.pair_inserts(ctg_lens, read_lens, alns, m)
                got = device_pairs(kc, read_lens, alns, m, **{off: False})
                if off != "want_hist":
                    assert got[0].tobytes() == w[0].tobytes()
                if off != "want_pairs":
                    assert got[1].tobytes() == w[1].tobytes()
                if off != "want_stats":
                    assert got[2] == w[2]
        # no records, and no reads
        out = compare(kc, ctg_lens, read_lens, records([]))
        assert out[2]["cls"] == [3, 0, 0, 0, 0, 0, 0] and not out[0].any()
        out = compare(kc, ctg_lens, [], records([]), 50)
        assert out[2]["pairs"] == 0 and len(out[0]) == 51
        # host arrays, inside canaries of their own
        offs = offsets_of(read_lens)
        h_hist = np.full(1001 + 2, 0xABABABABABABABAB, dtype=np.uint64)
        h_pairs = np.full((3 + 2) * 16, 0xAB, dtype=np.uint8)
        st = _lib.kc_insert_stats()
        rc = pkg.lib().kc_pair_inserts(kc._h, offs.ctypes.data, 6, alns.ctypes.data, len(alns), 0, 0, 0, 1000, h_hist.ctypes.data + 8,
                                       h_pairs.ctypes.data + 16, C.byref(st))
        assert rc == 0 and stats_dict(st) == want[2]
        assert h_hist[1:-1].tobytes() == want[0].tobytes() and h_pairs[16:-16].tobytes() == want[1].tobytes()
        assert h_hist[0] == h_hist[-1] == 0xABABABABABABABAB and (h_pairs[:16] == 0xAB).all() and (h_pairs[-16:] == 0xAB).all()
        # the wrapper, both modes
        h, p, s = kc.pair_inserts(offs, alns, max_insert=1000)
        assert h.dtype == np.uint64 and p.dtype == D.PAIR_DTYPE and (h.tobytes(), p.tobytes()) == (want[0].tobytes(), want[1].tobytes())
        assert {k: s[k] for k in STAT_FIELDS} == want[2] and s["mean"] == 240.0 and s["stddev"] == 0.0
        w = D.pair_inserts(ctg_lens, read_lens, alns, 239, 150, 100)
        d_alns = torch.from_numpy(np.frombuffer(alns.tobytes(), dtype=np.uint8).copy()).cuda()
        h, p, s = kc.pair_inserts(torch.from_numpy(offs.view(np.int64)).cuda(), d_alns, max_insert=239, min_score=150, min_len=100)
        assert h.is_cuda and p.is_cuda and h.cpu().numpy().view(np.uint64).tobytes() == w[0].tobytes()
        assert p.cpu().numpy().tobytes() == w[1].tobytes() and {k: s[k] for k in STAT_FIELDS} == w[2] and s["mean"] == 0.0
        # device record arrays are 16-byte aligned; the ranges, with a context this time
        assert device_pairs(kc, read_lens, alns, shift=8, expect=_lib.KC_ERR_INVALID_ARG) == _lib.KC_ERR_INVALID_ARG
        assert b"16-byte aligned" in pkg.lib().kc_last_error()
        device_pairs(kc, read_lens, alns, max_insert=0, expect=_lib.KC_ERR_INVALID_ARG)
        device_pairs(kc, read_lens, alns, max_insert=65536, expect=_lib.KC_ERR_INVALID_ARG)
        device_pairs(kc, read_lens[:5], alns[:6], expect=_lib.KC_ERR_INVALID_ARG)
        assert b"5 reads are no pairs" in pkg.lib().kc_last_error()
        # a read over the limit, named
        device_pairs(kc, read_lens[:3] + [1025] + read_lens[4:], alns, expect=_lib.KC_ERR_INVALID_ARG)
        assert b"kc_pair_inserts: read 3 " in pkg.lib().kc_last_error()
        compare(kc, ctg_lens, read_lens[:3] + [1024] + read_lens[4:], alns)


def test_names_and_launch_counts_in_the_kernel_times():
    ctg_lens, read_lens, alns = small_case()
    with lengths_index(ctg_lens, time_kernels=True) as kc:
        for max_insert, classify in ((1000, "kc_pair_classify_kernel<lds>"), (LDS_BINS, "kc_pair_classify_kernel")):  # LDS_BINS + 1 bins do not fit
            kc.kernel_times(clear=True)
            kc.pair_inserts(offsets_of(read_lens), alns, max_insert=max_insert)
            t = kc.kernel_times()
            want = {"kc_align_lengths_kernel<pair>": 1, "kc_depth_check_kernel<pair>": 1, "kc_depth_best_kernel<pair>": 1, classify: 1}
            assert {n: c for n, (c, _) in t.items()} == want


def test_invalid_records_are_named_and_nothing_is_written():
    ctg_lens, read_lens, alns = small_case()
    good = alns[3]  # read 2 of 100 bases on contig 0 (300 bases): cstart 200, cstop 300, rstart 0, rstop 100

    def forged(**kw):
        r = good.copy()
        for k, v in kw.items():
            r[k] = v
        return r

    none = records([NONE_REC])[0]
    bad = [forged(read=6), forged(read=0xFFFFFFFF), forged(ctg=3), forged(orient=2), forged(kind=3), forged(cstop=301), forged(cstart=300),
           forged(rstart=100), forged(rstop=101), forged(read=5, rstop=91), forged(read=4, rstart=0, rstop=1), forged(ctg=1, cstart=0, cstop=1),
           forged(read=6, kind=2)]
    none["read"] = 5
    ok = [forged(read=3, rstop=120, rstart=20), forged(read=5, rstop=90), none, forged(read=4, kind=2)]
    with lengths_index(ctg_lens) as kc:
        lib = pkg.lib()
        compare(kc, ctg_lens, read_lens, records(ok))
        for b in bad:
            with pytest.raises(D.BadRecord):
                D.pair_inserts(ctg_lens, read_lens, records([b]), 1000)
            assert device_pairs(kc, read_lens, records([b]), expect=_lib.KC_ERR_INVALID_ARG)
            assert b"kc_pair_inserts: record 0 " in lib.kc_last_error()
            many = np.concatenate([alns, alns[:1], records([b]), alns, records([b]), alns])
            with pytest.raises(D.BadRecord) as e:
                D.pair_inserts(ctg_lens, read_lens, many, 1000)
            assert e.value.index == 8
            device_pairs(kc, read_lens, many, expect=_lib.KC_ERR_INVALID_ARG)
            assert b"record 8 " in lib.kc_last_error()
        compare(kc, ctg_lens, read_lens, alns)


def test_state_rebuilt_index_and_ranks():
    ctg_lens, read_lens, alns = small_case()
    with pkg.KmerCounter(K) as kc:
        assert device_pairs(kc, read_lens, alns, expect=_lib.KC_ERR_STATE) == _lib.KC_ERR_STATE  # no index
    with lengths_index(ctg_lens) as kc:
        want = compare(kc, ctg_lens, read_lens, alns)
        kc.clear_contig_index()
        device_pairs(kc, read_lens, alns, expect=_lib.KC_ERR_STATE)
    with lengths_index(ctg_lens) as kc:
        kc.reset()
        device_pairs(kc, read_lens, alns, expect=_lib.KC_ERR_STATE)
    lens2 = [250, 301, 7]  # a rebuilt index with other lengths: the old records do not fit
    with lengths_index(ctg_lens) as kc:
        rng = np.random.default_rng(3)
        kc.index_contigs(*block_arrays([rand_seq(rng, n) for n in lens2]))
        device_pairs(kc, read_lens, alns, expect=_lib.KC_ERR_INVALID_ARG)
        alns2 = alns.copy()
        alns2["ctg"] = [1, 1, 0, 1, 1, 0, 0]
        got = compare(kc, lens2, read_lens, alns2)
        assert got[1].tobytes() == want[1].tobytes()
    with lengths_index(ctg_lens, rank_me=1, rank_n=2) as kc:
        compare(kc, ctg_lens, read_lens, alns)
