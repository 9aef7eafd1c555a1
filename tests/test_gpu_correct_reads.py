"""kc_correct_reads on the device equals tests/correct_model.py byte for byte -- out, records, fixes and statistics -- and
the answers that follow from the constructions of tests/correct_cases.py alone.  The model's table is
the oracle's results, not the device's.  Shapes: a 3000-base genome under 200 tiled reads a k; the block of a k holds every
planted case and every reason, the read lengths around k, empty sequences, 3000 clean reads of k to k + 11 bases in a row
(several sequences in a lane's 16 positions, and no weak window), and sequences past a lane's, a wave's (1024) and a
workgroup's (4096) positions with an error every 170 bytes -- about 120 to 360 KB.  One sequence of 100 000 bases with an
error every 500 is 25 workgroups on one record."""
import ctypes as C

import numpy as np
import pytest
import torch

import correct_cases as CC
import correct_model as M
import kdepth_model as K
import mhm2_kmer_analysis_v2_amd as pkg
from mhm2_kmer_analysis_v2_amd import _lib

pytestmark = pytest.mark.gpu

KS = (21, 31, 32, 33, 64, 99)


def counter(k, length=3000, seed=0, **kw):
    """a finalized counter over the tiled reads of CC.counted(k), its results the oracle's"""
    _, _, (b, q, offs), (keys, counts), _ = CC.counted(k, length, seed)
    kc = pkg.KmerCounter(k, **kw)
    kc.submit_reads(b, q, offs)
    got = kc.sorted_results()
    if not kw:
        assert (got[0] == keys).all() and (got[1] == counts).all()
    return kc


def counts_of(k, length=3000, seed=0):
    return CC.cached(("counts", k, length, seed), lambda: M.Counts(CC.counted(k, length, seed)[4]))


def model(k, **kw):
    b, offs, _ = CC.block(k)
    return CC.cached(("model", k, tuple(sorted(kw.items()))), lambda: M.correct_reads(counts_of(k), k, b, offs, **kw))


def host(x):
    return x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy()


def same(got, want):
    out, recs, fixes, stats = got
    assert (host(out) == want[0]).all(), np.flatnonzero(host(out) != want[0])[:10]
    if recs is not None:
        r = host(recs).view(M.REC_DTYPE)
        for name in M.REC_DTYPE.names:
            assert (r[name] == want[1][name]).all(), (name, np.flatnonzero(r[name] != want[1][name])[:10], r[name][r[name] != want[1][name]][:10])
    if fixes is not None:
        f = host(fixes).view(M.FIX_DTYPE)
        assert len(f) == len(want[2])
        for name in M.FIX_DTYPE.names:
            assert (f[name] == want[2][name]).all(), (name, np.flatnonzero(f[name] != want[2][name])[:10])
    assert stats == want[3]


def on_device(b, offs):
    return torch.from_numpy(b).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()


@pytest.mark.parametrize("k", KS)
def test_block_equals_the_model(k):
    b, offs, _ = CC.block(k)
    with counter(k) as kc:
        want = model(k)  # the wrapper's defaults are the model's
        assert want[3]["accepted"] > 30 and want[3]["rounds"] == 3 and want[3]["weak_after"] > 0
        assert {M.THIN, M.UNANCHORED, M.SHORT_RUN, M.NO_GAIN} <= {1 << i for i in range(6) if (int(np.bitwise_or.reduce(want[1]["flags"])) >> i) & 1}
        same(kc.correct_reads(b, offs, with_fixes=True), want)
        same(kc.correct_reads(*on_device(b, offs), with_fixes=True), want)
        one = model(k, min_windows=1)
        assert one[3]["accepted"] > want[3]["accepted"] and int(np.bitwise_or.reduce(one[1]["flags"])) & M.AMBIGUOUS
        same(kc.correct_reads(b, offs, min_windows=1, with_fixes=True), one)
        # each optional output left out in turn: the others as before
        same(kc.correct_reads(b, offs, min_windows=1, with_records=False, with_fixes=True), one)
        same(kc.correct_reads(*on_device(b, offs), min_windows=1, with_records=True), one)
        same(kc.correct_reads(*on_device(b, offs), min_windows=1, with_records=False), one)
        prm = _lib.kc_correct_params(2, 8, 1, 3, 0, 0)
        out, recs, fixes = np.zeros(len(b), np.uint8), np.zeros(len(offs) - 1, M.REC_DTYPE), np.zeros(len(one[2]), M.FIX_DTYPE)
        assert pkg.lib().kc_correct_reads(kc._h, b.ctypes.data, None, len(b), offs.ctypes.data, len(offs) - 1, 0, C.byref(prm), out.ctypes.data,
                                          recs.ctypes.data, fixes.ctypes.data, len(fixes), None) == 0  # no stats; room for exactly the fixes
        same((out, recs, fixes, one[3]), one)
        # one round only
        first = model(k, min_windows=1, rounds=1)
        assert first[3]["rounds"] == 1 and 0 < first[3]["accepted"] < one[3]["accepted"]
        same(kc.correct_reads(b, offs, min_windows=1, rounds=1, with_fixes=True), first)
        same(kc.correct_reads(*on_device(b, offs), min_windows=1, rounds=1, with_fixes=True), first)


@pytest.mark.parametrize("k", (21, 64))
def test_one_long_sequence(k):
    G = CC.counted(k, 101_000, 1)[0]
    rng = np.random.default_rng(k)
    text = bytearray(G[500:100_500])
    plan = list(range(250, 100_000, 500))
    for p in plan:
        text[p] = CC.other_base(rng, text[p])
    b, offs = K.block([bytes(text), b"ACGT"])
    want = CC.cached(("long", k), lambda: M.correct_reads(counts_of(k, 101_000, 1), k, b, offs))
    assert want[0][:100_000].tobytes() == G[500:100_500] and want[3]["accepted"] == len(plan) == 200 and want[3]["rounds"] == 2
    assert want[1][0]["corrected"] == 200 and want[1][0]["weak_before"] == 200 * k
    with counter(k, 101_000, 1) as kc:
        same(kc.correct_reads(b, offs, with_fixes=True), want)
        same(kc.correct_reads(*on_device(b, offs), with_fixes=True), want)


@pytest.mark.parametrize("k", (21, 33, 99))
def test_planted_reads_come_back_by_construction(k):
    """no model: out is the error-free read wherever the plan says so, and every window of those reads is solid"""
    cases = CC.planted_cases(k)
    b, offs = K.block([c[1] for c in cases])
    with counter(k) as kc:
        out, recs, fixes, stats = kc.correct_reads(b, offs, min_windows=1, with_fixes=True)
        assert out.tobytes() == b"".join(c[2] for c in cases)
        plan = [(i, p, old, new) for i, c in enumerate(cases) for p, old, new in c[3]]
        assert sorted((int(f["seq"]), int(f["pos"]), int(f["old"]), int(f["new"])) for f in fixes) == plan
        assert [int(r["flags"]) for r in recs] == [c[4] for c in cases] and stats["accepted"] == len(plan)
        healed = [i for i, c in enumerate(cases) if c[2] != c[1] or not c[3] and not c[4]]
        _, drec, _ = kc.kmer_depths(out, offs, min_count=2)
        assert len(healed) > 15 and (drec["solid"][healed] == drec["windows"][healed]).all() and not recs["weak_after"][healed].any()
        assert (recs["weak_after"] == drec["windows"] - drec["solid"]).all()
        _, drec, _ = kc.kmer_depths(b, offs, min_count=2)
        assert (recs["weak_before"] == drec["windows"] - drec["solid"]).all()


@pytest.mark.parametrize("dev", (False, True))
def test_quality_gate_and_every_reason(dev):
    k = 33
    with counter(k) as kc:
        for name, read, quals, kw, why in CC.verdict_cases(k):
            b, offs = K.block([read])
            want = M.correct_reads(counts_of(k), k, b, offs, quals=quals, **kw)
            assert want[1][0]["flags"] == why
            args = on_device(b, offs) if dev else (b, offs)
            q = quals if quals is None or not dev else torch.from_numpy(quals).cuda()
            same(kc.correct_reads(*args, quals=q, with_fixes=True, **kw), want)
        name, read, quals, kw, why = CC.verdict_cases(k)[5]
        b, offs = K.block([read])
        args = on_device(b, offs) if dev else (b, offs)
        q = torch.from_numpy(quals).cuda() if dev else quals
        for max_qual in (0, 29, 30):
            want = M.correct_reads(counts_of(k), k, b, offs, quals=quals, min_windows=1, max_qual=max_qual)
            assert want[3]["accepted"] == (max_qual != 29)
            same(kc.correct_reads(*args, quals=q, min_windows=1, max_qual=max_qual, with_fixes=True), want)


def poisoned(k, dev):
    """the planted block, its poisoned outputs on the caller's side and a call over them with room for `capacity` fixes"""
    cases = CC.planted_cases(k)
    b, offs = K.block([c[1] for c in cases])
    n = len(offs) - 1
    arrays = [np.full(len(b), 0xA5, np.uint8), np.full(n * 16, 0xA5, np.uint8), np.full(64 * 16, 0xA5, np.uint8)]
    st = _lib.kc_correct_stats(seqs=7, rounds=7)
    prm = _lib.kc_correct_params(2, 8, 1, 3, 0, 0)

    def call(kc, offsets, capacity):
        if dev:
            t = [torch.from_numpy(x).cuda() for x in [b, offsets.astype(np.int64)] + arrays]
            torch.cuda.synchronize()
            rc = pkg.lib().kc_correct_reads(kc._h, t[0].data_ptr(), None, len(b), t[1].data_ptr(), n, 1, C.byref(prm), t[2].data_ptr(), t[3].data_ptr(),
                                            t[4].data_ptr(), capacity, C.byref(st))
            return rc, [x.cpu().numpy() for x in t[2:]]
        rc = pkg.lib().kc_correct_reads(kc._h, b.ctypes.data, None, len(b), offsets.ctypes.data, n, 0, C.byref(prm), arrays[0].ctypes.data,
                                        arrays[1].ctypes.data, arrays[2].ctypes.data, capacity, C.byref(st))
        return rc, arrays

    return cases, b, offs, st, call


@pytest.mark.parametrize("dev", (False, True))
def test_one_fix_too_many_is_refused_and_nothing_is_written(dev):
    k = 21
    cases, b, offs, st, call = poisoned(k, dev)
    fixes = sum(len(c[3]) for c in cases)
    assert 16 < fixes <= 64
    with counter(k) as kc:
        rc, arrays = call(kc, offs, fixes - 1)
        assert rc == _lib.KC_ERR_CAPACITY and b"kc_correct_reads: %d fixes, room for %d" % (fixes, fixes - 1) in pkg.lib().kc_last_error()
        assert all((x == 0xA5).all() for x in arrays) and (st.seqs, st.rounds, st.accepted) == (7, 7, 0)
        rc, arrays = call(kc, offs, fixes)
        assert rc == 0 and arrays[0].tobytes() == b"".join(c[2] for c in cases) and st.accepted == fixes and st.seqs == len(cases)
        assert (arrays[2][fixes * 16:] == 0xA5).all() and not (arrays[2][:fixes * 16] == 0xA5).all()


BAD_OFFSETS = [(lambda o: o.__setitem__(5, o[7] + 1), "kc_correct_reads: the offsets decrease behind sequence 5"),
               (lambda o: o.__setitem__(0, 1), "kc_correct_reads: the offsets of 21 sequences do not start at 0"),
               (lambda o: o.__setitem__(21, o[21] - 1), "kc_correct_reads: the offsets of 21 sequences do not end at nbytes"),
               (lambda o: o.__setitem__(21, o[21] + 1), "kc_correct_reads: the offsets of 21 sequences do not end at nbytes")]


@pytest.mark.parametrize("dev", (False, True))
def test_bad_offsets_are_refused_and_nothing_is_written(dev):
    k = 21
    cases, b, good, st, call = poisoned(k, dev)
    assert len(good) == 22
    with counter(k) as kc:
        for spoil, message in BAD_OFFSETS:
            offs = good.copy()
            spoil(offs)
            rc, arrays = call(kc, offs, 64)
            assert rc == _lib.KC_ERR_INVALID_ARG and message.encode() in pkg.lib().kc_last_error(), (message, pkg.lib().kc_last_error())
            assert all((x == 0xA5).all() for x in arrays) and (st.seqs, st.rounds, st.accepted) == (7, 7, 0)
        assert kc.correct_reads(b, good, min_windows=1)[0].tobytes() == b"".join(c[2] for c in cases)  # and the context still answers


def test_state_ranks_and_nothing_to_do():
    k = 21
    _, _, (rb, rq, ro), _, _ = CC.counted(k)
    b, offs, _ = CC.block(k)
    with pkg.KmerCounter(k) as kc:
        kc.submit_reads(rb, rq, ro)
        with pytest.raises(pkg.KcError) as e:
            kc.correct_reads(b, offs)
        assert e.value.status == _lib.KC_ERR_STATE and b"kc_correct_reads: no results (kc_finalize)" in pkg.lib().kc_last_error()
        kc.finalize()
        same(kc.correct_reads(b, offs, with_fixes=True), model(k))
        for seqs in ([], [b"", b"", b""]):
            eb, eo = K.block(seqs)
            same(kc.correct_reads(eb, eo, with_fixes=True), M.correct_reads(counts_of(k), k, eb, eo))
            same(kc.correct_reads(*on_device(eb, eo), with_fixes=True), M.correct_reads(counts_of(k), k, eb, eo))
        kc.reset()
        with pytest.raises(pkg.KcError) as e:
            kc.correct_reads(b, offs)
        assert e.value.status == _lib.KC_ERR_STATE
    with counter(k, rank_me=0, rank_n=2) as kc:
        with pytest.raises(pkg.KcError) as e:
            kc.correct_reads(b, offs)
        assert e.value.status == _lib.KC_ERR_INVALID_ARG and b"kc_correct_reads: rank_n is 2" in pkg.lib().kc_last_error()
    with pkg.KmerCounter(k) as kc:  # nothing was counted: every window is absent, every run unanchored
        kc.finalize()
        want = M.correct_reads({}, k, b, offs)
        assert want[3]["accepted"] == 0 and want[3]["weak_before"] == want[3]["windows"] > 1000
        same(kc.correct_reads(b, offs, with_fixes=True), want)


def test_the_results_are_left_alone():
    k = 33
    b, offs, _ = CC.block(k)
    keys = CC.counted(k)[3][0]
    queries = np.concatenate([keys[::7], keys[:5] ^ np.uint64(1 << 40)])
    with counter(k) as kc:
        text = kc.dump_text()  # sorts the results; from here on nothing may move them
        before = (kc.lookup(queries), kc.sorted_results(), kc.results(), kc.kmer_depths(b, offs, min_count=2)[:2])
        res = kc.finalize()
        ptrs = (res.d_keys, res.d_counts, res.n)
        same(kc.correct_reads(b, offs, with_fixes=True), model(k))
        same(kc.correct_reads(*on_device(b, offs), with_fixes=True), model(k))
        res = kc.finalize()
        assert (res.d_keys, res.d_counts, res.n) == ptrs and kc.dump_text() == text
        after = (kc.lookup(queries), kc.sorted_results(), kc.results(), kc.kmer_depths(b, offs, min_count=2)[:2])
        for x, y in zip(before, after):
            assert all((p == q).all() for p, q in zip(x, y))
