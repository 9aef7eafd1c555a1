"""kc_close_gaps on the device against tests/close_model.py: every output byte for byte with the model on the same input,
device arrays exactly sized inside canaries.  Records, scaffolds and members come from the models and the case builders
(tests/close_cases.py): nothing here runs kc_scaffold."""
import ctypes as C

import numpy as np
import pytest

import close_cases as CC
import close_model as M
import mhm2_kmer_analysis_v2_amd as pkg
import scaffold_model as SM
import test_close_model as T
from depth_model import rec, records
from mhm2_kmer_analysis_v2_amd import _lib
from test_gpu_aln_depths import PAD
from test_gpu_gap_align import block_arrays, read_arrays

pytestmark = pytest.mark.gpu

K = 21
OUTS = ("offsets", "scaffolds", "members", "closures", "stats")
INS = ("bases", "roffs", "alns", "scaf_in", "mem_in")
UNTOUCHED = dict(dict.fromkeys(M.CLOSE_STATS, 0), members=99)


def stats_dict(st):
    return {n: int(getattr(st, n)) for n in M.CLOSE_STATS}


@pytest.fixture(scope="module")
def kc():
    with pkg.KmerCounter(K) as c:
        yield c


def index(kc, contigs):
    kc.index_contigs(*block_arrays(contigs))
    return kc


def device_close(kc, case, want, expect=0, shift=0, rec_shift=0, capacity=None, query=False, skip=(), n_scaf=None, **kw):
    """the call on device arrays of exactly the size the model's result `want` has, inside canaries; shift: the block's and
    the read bytes' misalignment, rec_shift: the record arrays'.  Returns the outputs' host images in the model's order.
    expect != 0: the status is checked, and that nothing was written but, for KC_ERR_CAPACITY, the size and the statistics."""
    import torch
    seqs, offsets, scafs, members, closures, _ = want if want is not None else (b"", [0], [], [], [], None)
    b, o = read_arrays(case.reads)
    src = dict(bases=b.tobytes(), roffs=o.tobytes(), alns=case.alns.tobytes(), scaf_in=case.scaffolds.tobytes(), mem_in=case.members.tobytes())
    at_in = dict(bases=PAD + shift, roffs=PAD, alns=PAD + rec_shift, scaf_in=PAD + rec_shift, mem_in=PAD + rec_shift)
    h_in, d_in = {}, {}
    for n, raw in src.items():
        h_in[n] = np.full(len(raw) + 2 * PAD + 16, 0xCD, dtype=np.uint8)
        h_in[n][at_in[n]:at_in[n] + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        d_in[n] = torch.from_numpy(h_in[n]).cuda()
    sizes = dict(seqs=len(seqs), offsets=8 * len(offsets), scaffolds=32 * len(scafs), members=16 * len(members), closures=32 * len(closures))
    d = {n: torch.full((sz + 2 * PAD + 16,), 0xAB, dtype=torch.uint8, device="cuda") for n, sz in sizes.items()}
    at = dict(seqs=PAD + shift, offsets=PAD, scaffolds=PAD + rec_shift, members=PAD + rec_shift, closures=PAD + rec_shift)
    torch.cuda.synchronize()
    st, nb = _lib.kc_close_stats(members=99), C.c_uint64(0xABAB)
    p = _lib.kc_close_params(**M.params(**kw))
    ptr = lambda n: None if n in skip or (query and n == "seqs") else d[n].data_ptr() + at[n]
    pin = lambda n: d_in[n].data_ptr() + at_in[n]
    rc = pkg.lib().kc_close_gaps(kc._h, pin("bases"), pin("roffs"), len(case.reads), pin("alns") if len(case.alns) else None, len(case.alns),
                                 pin("scaf_in"), len(case.scaffolds) if n_scaf is None else n_scaf, pin("mem_in"), 1, C.byref(p), ptr("seqs"),
                                 sizes["seqs"] if capacity is None else capacity, ptr("offsets"), ptr("scaffolds"), ptr("members"),
                                 ptr("closures"), C.byref(nb), None if "stats" in skip else C.byref(st))
    h = {n: t.cpu().numpy() for n, t in d.items()}
    for n in INS:
        assert (d_in[n].cpu().numpy() == h_in[n]).all(), "the input %s was written" % n
    if expect or query:
        assert rc == expect, (rc, pkg.lib().kc_last_error())
        assert all((x == 0xAB).all() for x in h.values()), "a refused call or a size query wrote"
        if expect in (0, _lib.KC_ERR_CAPACITY):
            return int(nb.value), stats_dict(st)
        assert stats_dict(st) == UNTOUCHED and nb.value == 0xABAB, "a refused call wrote the size or the statistics"
        return rc
    assert rc == 0, pkg.lib().kc_last_error()
    out = {}
    for n, sz in sizes.items():
        if n in skip:
            assert (h[n] == 0xAB).all(), n
            out[n] = None
            continue
        assert (h[n][:at[n]] == 0xAB).all() and (h[n][at[n] + sz:] == 0xAB).all(), "a canary of %s was written" % n
        out[n] = h[n][at[n]:at[n] + sz].copy()
    if "stats" in skip:
        assert stats_dict(st) == UNTOUCHED
    return (out["seqs"], out["offsets"], out["scaffolds"], out["members"], out["closures"], None if "stats" in skip else stats_dict(st),
            int(nb.value))


def same(got, want, skip=()):
    assert got[6] == len(want[0])
    if "stats" not in skip:
        assert got[5] == want[5]
    for i, n in enumerate(("seqs",) + OUTS[:4]):
        if n in skip:
            continue
        w = np.frombuffer(want[i] if i == 0 else want[i].tobytes(), dtype=np.uint8)
        if got[i].tobytes() != w.tobytes():
            diff = np.nonzero(got[i] != w)[0]
            raise AssertionError("%s differs at %d bytes, first at %s: %s / %s" % (n, len(diff), diff[:8], got[i][diff[:8]], w[diff[:8]]))


def compare(kc, case, reindex=True, **kw):
    dev_kw = {k: kw.pop(k) for k in ("shift", "rec_shift", "skip") if k in kw}
    want = M.close_gaps(*case.args(), **kw)
    if reindex:
        index(kc, case.contigs)
    same(device_close(kc, case, want, **dev_kw, **kw), want, dev_kw.get("skip", ()))
    return want


# ---- the model's cases ----------------------------------------------------------------------------------------------------
def test_the_models_two_contig_cases(kc):
    for g in (1, 7, 63, 64, 65):
        for oa, ob in ((0, 0), (0, 1), (1, 0), (1, 1)):
            case = CC.two_contigs(g, oa, ob, old_join=20)
            want = compare(kc, case)
            assert M.strings(want) == [case.text]
    for seed in (1, 2):
        for case in (CC.chain(9, seed=seed), CC.chain(9, seed=seed, flip=True, reorder=seed + 50)):
            assert M.strings(compare(kc, case)) == [case.text]


def test_the_models_slack_thresholds_modes_and_votes(kc):
    case = CC.two_contigs(7)
    for x in case.alns:
        if x["ctg"] == 0:
            x["cstop"] -= 3
            x["rstop"] -= 3
        else:
            x["cstart"] += 3
            x["rstart"] += 3
    assert M.strings(compare(kc, case)) == [case.text]
    compare(kc, case, reindex=False, end_slack=2)
    case = CC.two_contigs(7, old_join=4)
    for kw in (dict(min_reads=3), dict(min_reads=4), dict(min_score=61), dict(min_len=31), dict(max_splint_gap=6), dict(max_read_alns=2)):
        compare(kc, case, **kw)
    index(kc, [T.A60, T.B70])
    case = CC.hand_case(T.A60, T.B70, ["ACG", "ACG", "ACG", "ACGTT"])
    assert [T.closure(compare(kc, case, reindex=False, min_agree_permille=x))["status"] for x in (750, 751)] == [M.FILLED, M.WEAK]
    for fills, back in ((["TTTTT", "ACG", "TTTTT", "ACG"], ()), (["ACG", "TTTTT", "ACG", "ACG", "GGGGGGG"], (1, 2)), (["TGCA", "ACGT"], ()),
                        (["gNNt-", "gNNCc", "TNNtc"], (2,)), (["NN", "N*"], (0,)), (["ACGTA", "ACGTA", "ACCTA", "TCGTA", "ACGTA"], (0, 2))):
        compare(kc, CC.hand_case(T.A60, T.B70, fills, backward=back), reindex=False)
        compare(kc, CC.hand_case(T.A60, T.B70, fills, backward=back), reindex=False, min_reads=1, min_agree_permille=0)


def test_the_models_abutments_overlaps_copied_joins_and_off_join_candidates(kc):
    assert T.closure(compare(kc, CC.two_contigs(0, old_join=11)))["status"] == M.ABUT
    assert T.closure(compare(kc, CC.two_contigs(-20, old_join=6)))["status"] == M.OVERLAP
    compare(kc, CC.two_contigs(-70, old_join=6, la=120, lb=100, flank=25), max_overlap=70)  # an overlap of more than one trip of 64
    spoiled = CC.two_contigs(-20, old_join=6)
    spoiled.contigs[1] = spoiled.contigs[1][:7] + "N" + spoiled.contigs[1][8:]
    assert T.closure(compare(kc, spoiled))["status"] == M.OVERLAP_REJECTED
    A = T.A60
    got = [T.closure(compare(kc, T.overlap_case(a, b, 25)))["status"] for a, b in ((A, A[-25:]), (A, A[-25:] + "G"), (A[-25:], "T" + A[-25:] + "G"))]
    assert got == [M.OVERLAP_REJECTED, M.OVERLAP, M.OVERLAP_REJECTED]
    for g, old in ((7, 0), (7, -3), (0, 0)):
        assert compare(kc, CC.two_contigs(g, old_join=old))[5]["cands_off_join"] == 3
    case = CC.hand_case(T.A60, T.B70, ["ACG", "ACG", "ACG"], extra_contigs=[CC.rand_seq(np.random.default_rng(9), 50)])
    case.alns = np.concatenate([case.alns, records([rec(0, 2, 10, 30, rstart=5, rstop=25)])])
    assert compare(kc, case, max_read_alns=2)[5]["reads_over_cap"] == 1
    rows = [rec(3, 1, 40, 70, rstart=0, rstop=30), rec(3, 0, 0, 30, rstart=33, rstop=63), rec(4, 0, 30, 60, rstart=0, rstop=30),
            rec(4, 2, 0, 30, rstart=32, rstop=62), rec(5, 0, 30, 60, rstart=0, rstop=30), rec(5, 1, 40, 70, rstart=0, rstop=30, orient=1)]
    case.alns = np.concatenate([case.alns[:6], records(rows)])
    case.reads += ["A" * 63] * 3
    assert compare(kc, case, reindex=False)[5]["cands_off_join"] == 3
    case = CC.hand_case(T.A60, T.B70, ["ACG", "ACG"])
    case.scaffolds = CC.scaffold_records([2], flags=[SM.CIRCULAR])
    case.alns = np.concatenate([case.alns, records([rec(2, 1, 40, 70, rstart=0, rstop=30), rec(2, 0, 0, 30, rstart=33, rstop=63)])])
    case.reads.append("C" * 63)
    assert int(compare(kc, case)[2][0]["flags"]) == SM.CIRCULAR


@pytest.mark.parametrize("name", ["gaps", "overlap"])
def test_the_models_construction_closes_to_the_genome(kc, name):
    G, links, case = T.layout_case(name)
    want = compare(kc, case, **T.LINK_KW)
    assert M.strings(want) == [G] and want[5]["n_bases_left"] == 0


# ---- the vote and the writer at their edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [1, 15, 16, 17, 63, 64, 65, 255, 900])
def test_fill_lengths(kc, g):
    case = CC.two_contigs(g, la=61, seed=g, supporters=5, backward=2, old_join=3, flank=40)
    assert max(len(r) for r in case.reads) <= 1024
    for i in (1, 3):  # a substitution in a forward and in a backward supporter: the fill's first column and its last
        col = 40
        t = case.reads[i]
        case.reads[i] = t[:col] + CC.revc(t[col]) + t[col + 1:]
    want = compare(kc, case, max_splint_gap=1024)
    assert M.strings(want) == [case.text] and T.closure(want)["disputed"] == (1 if g == 1 else 2)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 3000])
def test_supporters_on_one_join_and_the_tile_scans_edges_over_the_reads(kc, n):
    case = CC.two_contigs(9, seed=n, supporters=n, backward=n // 3)
    for i in range(3, n, 7):  # every seventh read disagrees in one column; where they meet they are outvoted or win the tie to A C G T
        col = 30 + i % 9
        case.reads[i] = case.reads[i][:col] + "T" + case.reads[i][col + 1:]
    for i in range(5, n, 11):  # and every eleventh claims another distance
        case.alns[2 * i + 1]["rstart"] += 1
    want = compare(kc, case, min_reads=1)
    assert want[5]["cands"] == n and T.closure(want)["status"] == M.FILLED


def test_the_fill_and_the_member_behind_it_at_every_destination_alignment(kc):
    fills, behind = set(), set()
    for a in range(16):  # the fill starts at byte 60 + a of an aligned block, the member behind it at 67 + a
        case = CC.two_contigs(7, la=60 + a, seed=a)
        want = compare(kc, case)
        fills.add(T.closure(want)["fill_pos"] % 16)
        behind.add(int(want[3][1]["out_pos"]) % 16)
        compare(kc, case, reindex=False, shift=(5 * a + 3) % 16)  # and the block itself misaligned
    assert fills == behind == set(range(16))


@pytest.mark.parametrize("n", [2, 1023, 1024, 1025, 4097])
def test_chains_with_a_gap_at_every_join(kc, n):
    case = CC.chain(n, seed=n)
    want = compare(kc, case)
    assert M.strings(want) == [case.text] and want[5]["filled"] == n - 1
    if n == 1025:  # as many scaffolds as the members allow, and a few
        case.scaffolds = CC.scaffold_records([1] * 500 + [25] * 21)
        for m in set(np.cumsum([0] + [1] * 500 + [25] * 20).tolist()):
            case.members[m]["join"] = 0
        compare(kc, case, reindex=False, shift=3)


def test_short_members_and_fills_inside_one_chunk(kc):
    case = CC.chain(300, seed=12, lens=(22, 26), gaps=(1, 3), flank=21)
    want = compare(kc, case)
    assert {int(c["fill_pos"]) % 16 for c in want[4]} == set(range(16)) and M.strings(want) == [case.text]


# ---- degenerate inputs, optional outputs, capacity ------------------------------------------------------------------------
def test_no_gap_joins_no_records_no_reads_and_empty_contigs(kc):
    case = CC.chain(20, seed=5)
    for m in range(1, 20):
        case.members[m]["join"] = 0 if m & 1 else -2
    want = compare(kc, case)
    assert want[5]["gaps"] == 0 and want[5]["cands_off_join"] == want[5]["cands"] == 38
    case = CC.chain(20, seed=5)
    case.alns = case.alns[:0]
    assert compare(kc, case, reindex=False)[5]["gaps_no_reads"] == 19
    case.reads = []
    compare(kc, case, reindex=False)
    members = np.array([(0, 0, 0, 0, (0, 0, 0)), (1, 0, 0, 1, (0, 0, 0)), (2, 2, 0, 0, (0, 0, 0))], dtype=SM.MEMBER_DTYPE)
    compare(kc, CC.Case(None, ["ACG", "", "T"], [], records([]), CC.scaffold_records([1, 2]), members))
    compare(kc, CC.Case(None, [""], [], records([]), CC.scaffold_records([1]), members[:1]))


def small_case():
    return CC.chain(12, seed=8)


def test_each_optional_output_null_in_turn_the_size_query_and_the_capacity(kc):
    case = small_case()
    want = M.close_gaps(*case.args())
    index(kc, case.contigs)
    for n in OUTS:
        same(device_close(kc, case, want, skip=(n,)), want, skip=(n,))
    same(device_close(kc, case, want, skip=OUTS), want, skip=OUTS)
    counts = (len(want[0]), want[5])
    assert device_close(kc, case, want, query=True) == counts
    assert device_close(kc, case, want, query=True, skip=("stats",))[0] == counts[0]
    for cap in (len(want[0]) - 1, 0):
        assert device_close(kc, case, want, expect=_lib.KC_ERR_CAPACITY, capacity=cap) == counts
        assert b"kc_close_gaps: %d bytes, the array holds %d" % (len(want[0]), cap) in pkg.lib().kc_last_error()
    same(device_close(kc, case, want, capacity=len(want[0]) + 100), want)


def test_host_arrays_device_tensors_and_the_wrapper_twice(kc):
    import torch
    case = small_case()
    want = M.close_gaps(*case.args())
    index(kc, case.contigs)
    b, o = read_arrays(case.reads)
    host = (b, o, case.alns, case.scaffolds, case.members)
    dev = tuple(torch.from_numpy(np.frombuffer(x.tobytes(), dtype=np.uint8 if i != 1 else np.int64).copy()).cuda() for i, x in enumerate(host))
    for _ in range(2):
        res = kc.close_gaps(*host)
        assert [x.tobytes() for x in res[:5]] == [want[0]] + [x.tobytes() for x in want[1:5]] and res[5] == want[5]
        assert res[2].dtype == pkg.kcount.SCAFFOLD_DTYPE and res[3].dtype == pkg.kcount.MEMBER_DTYPE and res[4].dtype == pkg.kcount.CLOSURE_DTYPE
        res = kc.close_gaps(*dev)
        assert all(x.is_cuda for x in res[:5]) and res[5] == want[5]
        assert [x.cpu().numpy().tobytes() for x in res[:5]] == [want[0]] + [x.tobytes() for x in want[1:5]]
        assert kc.close_gaps_strings(*dev) == M.strings(want) == kc.close_gaps_strings(*host) == [case.text]
    # index_contigs takes the closed block as it is
    kc.index_contigs(res[0], res[1])
    assert kc.contig_index_info() == (len(want[0]), 1)


# ---- invalid input and the order of the checks ---------------------------------------------------------------------------------
def test_invalid_input_is_named_in_the_order_of_the_checks_and_nothing_is_written(kc):
    good = T.chain5()
    want = M.close_gaps(*good.args())
    index(kc, good.contigs)
    err = lambda: pkg.lib().kc_last_error()
    for name, spoil in T.bad_scaffolds():
        for idx in ((1,), (3,), (3, 1), (0,)):
            case = T.chain5()
            case.scaffolds = CC.scaffold_records([1, 1, 1, 1, 1])
            for m in range(5):
                case.members[m]["join"] = 0
            for i in idx:
                spoil(case.scaffolds, i)
            device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG)
            assert b"kc_close_gaps: scaffold %d is invalid" % min(idx) in err(), (name, idx, err())
    for counts, bad in (([5, 1], 1), ([2, 2], 1), ([2, 4], 1), ([1, 1, 1, 1, 1, 1], 5)):
        case = T.chain5()
        case.scaffolds = CC.scaffold_records(counts)
        device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG)
        assert b"kc_close_gaps: scaffold %d is invalid" % bad in err(), (counts, err())
    device_close(kc, good, want, expect=_lib.KC_ERR_INVALID_ARG, n_scaf=0)
    assert b"kc_close_gaps: scaffold 0 is invalid" in err()
    for k in range(7):
        for idx in ((2,), (4,), (4, 2)):
            case = T.chain5()
            name, spoil = list(T.bad_members(case))[k]
            for i in idx:
                spoil(case.members, i)
            device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG)
            assert b"kc_close_gaps: member %d is invalid" % min(idx) in err(), (name, idx, err())
    case = T.chain5()
    case.members[0]["join"] = 3
    device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG)
    assert b"kc_close_gaps: member 0 is invalid" in err()
    # the order: parameters, alignment, reads, records, scaffolds, members
    case = T.chain5()
    case.members[3]["orient"] = 2
    case.scaffolds = CC.scaffold_records([2, 2])
    case.alns[4]["ctg"] = 9
    case.reads[1] = "A" * 1025
    device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG, min_reads=0, rec_shift=8)
    assert b"min_reads 0 below 1" in err()
    device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG, rec_shift=8)
    assert b"kc_close_gaps: a device record array is 16-byte aligned" in err()
    device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG)
    assert b"kc_close_gaps: read 1 is longer than 1024 bases" in err()
    case.reads[1] = "A" * 1024
    device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG)
    assert b"kc_close_gaps: record 4 is not a valid kc_gap_aln" in err()
    case.alns[4]["ctg"] = 0
    device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG)
    assert b"kc_close_gaps: scaffold 1 is invalid" in err()
    case.scaffolds = CC.scaffold_records([5])
    device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG)
    assert b"kc_close_gaps: member 3 is invalid" in err()
    same(device_close(kc, good, want), want)


def test_index_states_and_ranks():
    case = T.chain5()
    want = M.close_gaps(*case.args())
    with pkg.KmerCounter(K) as kc:
        device_close(kc, case, want, expect=_lib.KC_ERR_STATE)  # no index
        assert b"kc_close_gaps: no contig index" in pkg.lib().kc_last_error()
        index(kc, case.contigs)
        same(device_close(kc, case, want), want)
        kc.clear_contig_index()
        device_close(kc, case, want, expect=_lib.KC_ERR_STATE)
        index(kc, case.contigs[:4])  # a rebuilt index with four contigs: the records of the fifth are invalid now
        device_close(kc, case, want, expect=_lib.KC_ERR_INVALID_ARG)
        assert b"is not a valid kc_gap_aln" in pkg.lib().kc_last_error()
        index(kc, case.contigs)
        same(device_close(kc, case, want), want)
        kc.reset()
        device_close(kc, case, want, expect=_lib.KC_ERR_STATE)
    with pkg.KmerCounter(K, rank_me=1, rank_n=2) as kc:
        index(kc, case.contigs)
        same(device_close(kc, case, want), want)


def test_names_and_launch_counts_in_the_kernel_times():
    case = CC.chain(65, seed=3)
    b, o = read_arrays(case.reads)
    with pkg.KmerCounter(K, time_kernels=True) as kc:
        index(kc, case.contigs)
        kc.kernel_times(clear=True)
        kc.close_gaps(b, o, case.alns, case.scaffolds, case.members)  # a size query and the call
        t = kc.kernel_times()
    want = {"kc_align_lengths_kernel<close>": 2, "kc_depth_check_kernel<close>": 2, "kc_close_check_scaf_kernel": 2, "kc_close_claim_kernel": 2,
            "kc_close_check_member_kernel": 2, "kc_link_group_kernel<close count>": 2, "kc_link_group_kernel<close fill>": 2,
            "kc_link_tile_scan_kernel<close>": 8, "kc_close_scan_kernel": 8, "kc_close_ends_kernel": 2, "kc_close_cands_kernel<count>": 2,
            "kc_close_cands_kernel<write>": 2, "kc_close_decide_kernel": 2, "kc_close_place_kernel": 2, "kc_close_vote_kernel": 2,
            "kc_close_records_kernel": 1, "kc_close_write_kernel": 1}
    assert {n: c for n, (c, _) in t.items()} == want
