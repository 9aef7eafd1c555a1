"""tests/break_model.py held to cases whose answer follows from the case alone (no GPU needed), the geometry the GPU cases of
tests/break_cases.py claim, and the ground truth of the chain case: computed here through the host models align_model, gap_model
and depth_model, which proves that the chosen seed does what tests/test_gpu_ctg_break_chain.py claims (gap_model's dynamic
programme in Python over 4000 reads is what that one test costs)."""
import functools

import numpy as np
import pytest

import align_model as A
import break_cases as BC
import break_model as M
import depth_model as DM
import gap_model as GM
from links_cases import K, READ_LEN

T = BC.T


def small(L=10, n=200, **kw):
    c = BC.Case(1, L=L, **dict(dict(max_insert=40, margin=3, min_disc=1), **kw))
    c.contig(BC.DUMP)
    c.contig(n)
    return c


def track(out, which, u=1, c=None):
    """a track of contig 1 (the block's bytes behind the dump contig)"""
    return out[6][which][BC.DB:-1].astype(int)


def interval(t):
    nz = np.flatnonzero(t)
    assert len(nz) and (np.diff(nz) == 1).all()
    return int(nz[0]), int(nz[-1]) + 1


def test_one_spanning_pair():
    c = small()
    c.span(1, 50, 85)
    out = c.model()
    assert interval(track(out, 0)) == (50, 85) and not track(out, 1).any()
    assert (out[5]["spanning"], out[5]["span_sum"], out[5]["disc_mates"], out[5]["breaks"]) == (1, 35, 0, 0)
    assert out[0] == c.contig_block()[0].tobytes() and (out[1] == c.contig_block()[1]).all() and (out[2] == c.depths()).all()
    assert out[3].tolist() == [(0, 0, BC.DUMP, 0), (1, 0, 200, 0)] and len(out[4]) == 0


def test_every_pair_class_and_both_orients():
    want = BC.expected("classes")[5]
    assert (want["pairs"], want["spanning"], want["discordant_pairs"], want["one_mate"], want["none"]) == (16, 4, 8, 2, 2)
    assert want["disc_mates"] == 16 and want["empty_intervals"] == 0
    assert BC.case("classes").model(one_mate=True)[5]["disc_mates"] == 18
    for orient, at, lo, hi in ((0, 60, 60, 100), (1, 60, 20, 60)):  # the window lies ahead of a forward mate, behind a reverse one
        c = small()
        c.disc(1, at, orient)
        out = c.model()
        assert interval(track(out, 1)) == (lo, hi) and out[5]["discordant_pairs"] == 1 and out[5]["disc_mates"] == 2
    c = small()  # the reverse mate is read 0: F and R are chosen by orient, not by order
    c.pair(c.rev(1, 95), c.fwd(1, 65))
    assert interval(track(c.model(), 0)) == (65, 95)


def test_clamps_at_both_contig_ends():
    c = small(n=120)
    c.pair(dict(ctg=1, cstart=0, cstop=6, orient=0, rstart=4), dict(ctg=1, cstart=14, cstop=20, orient=1, rstart=0, rstop=6))  # fs = -4, re = 24
    c.pair(c.fwd(1, 100), dict(ctg=1, cstart=112, cstop=120, orient=1, rstart=0, rstop=8))  # re = 122
    out = c.model()
    t = track(out, 0)
    assert out[5]["spanning"] == 2 and (t[:24] == 1).all() and (t[24:100] == 0).all() and (t[100:] == 1).all() and out[5]["span_sum"] == 44
    c = small(n=120)
    c.pair(dict(ctg=1, cstart=0, cstop=5, orient=0, rstart=5), c.dumpmate())  # s = -5: [0, 35)
    c.pair(c.dumpmate(), dict(ctg=1, cstart=112, cstop=120, orient=1, rstart=0, rstop=8))  # e = 122: [82, 120)
    t = track(c.model(), 1)
    assert (t[:35] == 1).all() and (t[35:82] == 0).all() and (t[82:] == 1).all()
    c = small(n=120, max_insert=3)  # s + max_insert <= 0: an empty interval, counted and not added
    c.pair(dict(ctg=1, cstart=0, cstop=5, orient=0, rstart=5), None)
    out = c.model(one_mate=True)
    assert (out[5]["disc_mates"], out[5]["empty_intervals"], out[5]["disc_sum"]) == (0, 1, 0)


def test_everted_and_one_over_max_insert_turn_both_mates_discordant():
    for pair, proper in ((lambda c: (c.fwd(1, 50), c.rev(1, 90)), True), (lambda c: (c.fwd(1, 50), c.rev(1, 91)), False),
                         (lambda c: (c.fwd(1, 120), c.rev(1, 125)), False), (lambda c: (c.fwd(1, 50), c.fwd(1, 70)), False)):
        c = small()
        c.pair(*pair(c))
        st = c.model()[5]
        assert (st["spanning"], st["discordant_pairs"], st["disc_mates"]) == ((1, 0, 0) if proper else (0, 1, 2))


def test_one_mate_on_and_off():
    c = small()
    c.pair(c.fwd(1, 50), None)
    c.pair(None, c.rev(1, 150))
    off, on = c.model(), c.model(one_mate=True)
    assert off[5]["one_mate"] == on[5]["one_mate"] == 2 and off[5]["disc_mates"] == 0 and not track(off, 1).any()
    assert on[5]["disc_mates"] == 2 and on[5]["disc_sum"] == 80 and (track(on, 1)[[50, 89, 110, 149]] == 1).all() and not track(on, 1)[[49, 90, 109, 150]].any()


def test_margin_bounds_of_a_run():
    """disc everywhere: the weak columns are exactly margin <= i < len - margin; column margin - 1 never is"""
    for n, margin in ((60, 7), (15, 7), (14, 7), (13, 7)):
        c = small(L=4, n=n, max_insert=64, margin=margin)
        c.disc(1, 0, 0)
        out = c.model()
        lo, hi = margin, n - margin
        if n <= 2 * margin:
            assert out[5]["weak"] == 0 == out[5]["interior"] and len(out[4]) == 0
        else:
            b = out[4][0]
            assert (int(b["run_start"]), int(b["run_len"]), int(b["pos"])) == (lo, hi - lo, lo + (hi - lo) // 2) and out[5]["weak"] == hi - lo
            assert out[3].tolist()[1:] == [(1, 0, int(b["pos"]), 2), (1, int(b["pos"]), n - int(b["pos"]), 1)]


def test_min_run_two_runs_parted_by_one_column_and_m_for_odd_and_even_lengths():
    c = BC.case("parted")  # holes of 3, 2, 3, 4, 5, 6, 7 columns; min_run is 4
    out = BC.expected("parted")
    assert out[5]["runs"] == 7 and out[5]["short_runs"] == 3 and out[5]["breaks"] == 4
    assert [(int(b["run_start"]), int(b["run_len"]), int(b["pos"])) for b in out[4]] == [(150, 4, 152), (200, 5, 202), (250, 6, 253), (300, 7, 303)]
    low = c.model(min_run=2)  # runs of 3 and 2 parted by the one spanned column 53 stay two runs
    assert [(int(b["run_start"]), int(b["run_len"]), int(b["pos"])) for b in low[4]][:3] == [(50, 3, 51), (54, 2, 55), (100, 3, 101)]
    assert c.model(min_run=3)[5]["breaks"] == 6 and c.model(min_run=8)[5]["breaks"] == 0
    texts = out[0].decode().split("_")[:-1]
    assert "".join(texts[1:]) == c.contigs[1] and [len(t) for t in texts[1:]] == [152, 50, 51, 50, 97]
    assert [int(b["piece"]) for b in out[4]] == [2, 3, 4, 5] and out[3]["flags"].tolist() == [0, 2, 3, 3, 3, 1]
    assert (out[1] == np.concatenate(([0], np.cumsum([len(t) + 1 for t in texts])))).all()
    d = c.depths()
    assert (out[2][out[1][2] - 1:out[1][2] + 2] == [0, d[BC.DB + 152], d[BC.DB + 153]]).all() and out[2][out[1][1]] == d[BC.DB]


def test_thresholds_of_the_levels_case():
    c = BC.case("levels")
    weak = lambda **kw: c.model(**kw)[5]["weak"]  # noqa: E731
    # span k on 20 columns under disc 3, k = 0 .. 4 (min_disc 2): a column joins when max_span reaches its span, not before
    assert [weak(max_span=k) - weak(max_span=k - 1) for k in range(2, 5)] == [20] * 3 and weak(max_span=5) == weak(max_span=4) > weak(max_span=0) > 0
    # disc 3 on five windows of 32 columns and disc k on five more, k = 0 .. 4: a column leaves when min_disc passes its disc
    assert [weak(max_span=9, min_disc=k) for k in range(6)] == [600 - 2 * 2, 9 * 32, 8 * 32, 7 * 32, 32, 0]


def test_saturation_is_of_the_tracks_only():
    out = BC.expected("saturate")
    sp, di = out[6]
    at = lambda k: BC.DB + k  # noqa: E731
    assert [int(sp[at(x)]) for x in (120, 220, 320)] == [65535, 65535, 65535] and [int(di[at(x)]) for x in (620, 720, 820)] == [65535] * 3
    assert out[5]["span_sum"] == 40 * (65535 + 65536 + 70000) and out[5]["disc_sum"] == 64 * (65535 + 65536 + 70000)
    assert [(int(b["run_start"]), int(b["disc"]), int(b["span"])) for b in out[4]] == [(700, 65536, 0), (800, 70000, 0)]


def test_the_gpu_cases_have_the_geometry_they_claim():
    """block positions: m, the runs' ends, the separators"""
    def blockpos(name):
        c, out = BC.case(name), BC.expected(name)
        o = c.contig_block()[1]
        return [(int(o[b["ctg"]]) + int(b["run_start"]), int(o[b["ctg"]]) + int(b["run_start"]) + int(b["run_len"]), int(o[b["ctg"]]) + int(b["pos"]))
                for b in out[4]], len(c.contig_block()[0])

    for name, n in (("size_t-1", T - 1), ("size_t", T), ("size_t+1", T + 1), ("size_3t+1", 3 * T + 1)):
        runs, nbytes = blockpos(name)
        assert nbytes == n and len(runs) == 3 and runs[0][0] == BC.DB + 4 and runs[2][1] == n - 1 - 4
    assert blockpos("tile_last")[0][0][1] == T  # its last column is byte T - 1
    assert [r[0] for r in blockpos("tile_first")[0]] == [T, 2 * T]
    (a, b, _), = blockpos("three_tiles")[0]
    assert a < T and b > 2 * T and (a // T, (b - 1) // T) == (0, 2)
    assert sorted(r[2] for r in blockpos("cut_tile_first")[0]) == [T, 2 * T]
    c = BC.case("sep_tile_last")
    assert int(c.contig_block()[1][2]) - 1 == T - 1 and sum(1 for b in BC.expected("sep_tile_last")[4] if b["ctg"] == 1) == 2
    out = BC.expected("margins")
    assert [int(b["ctg"]) for b in out[4]] == [2, 4] and [int(b["pos"]) for b in out[4]] == [4, 4] and out[5]["weak"] == 2
    assert len(BC.case("empties").contigs) == 303 and BC.expected("empties")[5]["breaks"] == 3
    c, out = BC.case("many"), BC.expected("many")
    big = [u for u, x in enumerate(c.contigs) if len(x) == 300020]
    assert len(c.contigs) == 5002 and len(big) == 1 and sum(1 for b in out[4] if b["ctg"] == big[0]) == 3 and out[5]["broken_contigs"] == 53 and out[5]["breaks"] == 55
    for n in (0, 1, 17, 4097):
        out = BC.expected("gather%d" % n)
        assert out[5]["breaks"] == n and len(out[0]) == len(BC.case("gather%d" % n).contig_block()[0]) + n
    seps = np.flatnonzero(np.frombuffer(BC.expected("gather4097")[0], dtype=np.uint8) == ord("_"))
    assert set((seps % 16).tolist()) == set(range(16))  # the inserted separators meet the 16-byte chunks at every offset
    assert BC.expected("none")[5]["none"] == 5 and BC.expected("none")[0] == BC.case("none").contig_block()[0].tobytes()


# ---- the chain case's ground truth, through the host models -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_chain():
    c = BC.chain_case()
    index = A.Index(*A.join_block(c.contigs), K)
    alns = A.align_reads(index, c.reads)[0]
    gapped, _ = GM.align_gapped(c.contigs, c.reads, alns)
    _, pairs, ist = DM.pair_inserts(c.ctg_lens, c.read_lens, gapped, max_insert=BC.CHAIN_INSERT)
    return c, gapped, pairs, ist, M.break_contigs(c.contigs, c.read_lens, gapped, pairs, **BC.CHAIN_KW)


def test_the_chain_case_breaks_the_chimeric_contig_once_and_nothing_else():
    c, gapped, pairs, ist, out = model_chain()
    assert [len(x) for x in c.contigs] == [5000, 2500, 2500] and c.junction == 2500 and len(c.reads) == 4000
    st = out[5]
    assert st["breaks"] == 1 == st["broken_contigs"] and st["pieces"] == 4
    b = out[4][0]
    assert int(b["ctg"]) == 0
    distance = abs(int(b["pos"]) - c.junction)
    print("the break at %d, the junction at %d: %d apart; the run [%d, %d); %s" % (b["pos"], c.junction, distance, b["run_start"],
                                                                                  b["run_start"] + b["run_len"], st))
    assert distance <= READ_LEN
    assert out[3].tolist() == [(0, 0, int(b["pos"]), 2), (0, int(b["pos"]), 5000 - int(b["pos"]), 1), (1, 0, 2500, 0), (2, 0, 2500, 0)]
    # every pair is proper or has its mates on two contigs, and only pairs across the junction do
    assert ist["cls"][DM.PAIR_PROPER] + ist["cls"][DM.PAIR_DIFF_CTG] == 2000 and st["discordant_pairs"] == ist["cls"][DM.PAIR_DIFF_CTG] > 50
    # the true contigs' interiors hold no discordant mate at all
    o = np.cumsum([0] + [len(x) + 1 for x in c.contigs])
    for u in (1, 2):
        assert not out[6][1][o[u] + BC.CHAIN_INSERT:o[u] + 2500 - BC.CHAIN_INSERT].any()


@pytest.mark.parametrize("name", sorted(BC.BUILDERS))
def test_every_case_is_valid_input(name):
    """what the device checks: the records by depth_model's validity, the pairs by kc_local_assm's rule"""
    c = BC.case(name)
    lens = [int(x) for x in c.arrays()[2]]
    alns, pairs = c.alns, c.pairs
    step = max(1, len(alns) // 2000)  # the bulk records are copies of one another
    for i in list(range(0, len(alns), step)) + [len(alns) - 1] * bool(len(alns)):
        assert DM.valid(alns[i], [len(x) for x in c.contigs], lens, len(lens)), (name, i, alns[i])
    assert len(pairs) * 2 == len(lens)
    for f, side in (("aln0", 0), ("aln1", 1)):
        has = pairs[f] != M.NO_ALN
        idx = pairs[f][has]
        assert (idx < len(alns)).all() and (alns["read"][idx] == 2 * np.flatnonzero(has) + side).all() and (alns["kind"][idx] != 2).all()
