"""kc_scaffold on the device against tests/scaffold_model.py: every output byte for byte with the model on the same input,
device arrays exactly sized inside canaries."""
import ctypes as C

import numpy as np
import pytest

import links_cases as LC
import mhm2_kmer_analysis_v2_amd as pkg
import scaffold_model as M
import test_scaffold_model as T
from mhm2_kmer_analysis_v2_amd import _lib
from scaffold_model import link, records
from test_gpu_aln_depths import PAD
from test_gpu_gap_align import block_arrays, read_arrays

pytestmark = pytest.mark.gpu

K = 21
OUTS = ("offsets", "scaffolds", "members", "ctg_member", "stats")


def stats_dict(st):
    return {n: int(getattr(st, n)) for n in M.SCAF_STATS}


UNTOUCHED = dict(dict.fromkeys(M.SCAF_STATS, 0), contigs=99)


@pytest.fixture(scope="module")
def kc():
    with pkg.KmerCounter(K) as c:
        yield c


def index(kc, contigs):
    kc.index_contigs(*block_arrays(contigs))
    return kc


def device_scaffold(kc, links, want, expect=0, shift=0, rec_shift=0, capacity=None, query=False, skip=(), **kw):
    """the call on device arrays of exactly the size the model's result `want` has, inside canaries; shift: the block's
    misalignment, rec_shift: the record arrays'.  Returns the outputs' host images in the model's order.  expect != 0: the
    status is checked, and that nothing was written but, for KC_ERR_CAPACITY, the counts and the statistics."""
    import torch
    seqs, offsets, scafs, members, ctg_member, _ = want if want is not None else (b"", [0], [], [], [], None)
    sizes = dict(seqs=len(seqs), offsets=8 * len(offsets), scaffolds=32 * len(scafs), members=16 * len(members), ctg_member=4 * len(ctg_member))
    d_links = torch.full((len(links) * 48 + 2 * PAD + 16,), 0xCD, dtype=torch.uint8, device="cuda")
    h_links = d_links.cpu().numpy()
    h_links[PAD + rec_shift:PAD + rec_shift + 48 * len(links)] = np.frombuffer(links.tobytes(), dtype=np.uint8)
    d_links = torch.from_numpy(h_links).cuda()
    d = {n: torch.full((sz + 2 * PAD + 16,), 0xAB, dtype=torch.uint8, device="cuda") for n, sz in sizes.items()}
    at = dict(seqs=PAD + shift, offsets=PAD, scaffolds=PAD + rec_shift, members=PAD + rec_shift, ctg_member=PAD)
    torch.cuda.synchronize()
    st, ns, nb = _lib.kc_scaf_stats(contigs=99), C.c_uint64(0xABAB), C.c_uint64(0xABAB)
    p = _lib.kc_scaf_params(**M.params(**kw))
    ptr = lambda n: None if n in skip or (query and n == "seqs") else d[n].data_ptr() + at[n]
    rc = pkg.lib().kc_scaffold(kc._h, d_links.data_ptr() + PAD + rec_shift if len(links) else None, len(links), 1, C.byref(p), ptr("seqs"),
                               sizes["seqs"] if capacity is None else capacity, ptr("offsets"), ptr("scaffolds"), ptr("members"),
                               ptr("ctg_member"), C.byref(ns), C.byref(nb), None if "stats" in skip else C.byref(st))
    h = {n: t.cpu().numpy() for n, t in d.items()}
    assert (d_links.cpu().numpy() == h_links).all(), "the input records were written"
    if expect or query:
        assert rc == expect, (rc, pkg.lib().kc_last_error())
        assert all((x == 0xAB).all() for x in h.values()), "a refused call or a size query wrote"
        if expect in (0, _lib.KC_ERR_CAPACITY):
            return int(ns.value), int(nb.value), stats_dict(st)
        assert stats_dict(st) == UNTOUCHED and (ns.value, nb.value) == (0xABAB, 0xABAB), "a refused call wrote the counts or the statistics"
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
    return (out["seqs"], out["offsets"], out["scaffolds"], out["members"], out["ctg_member"], None if "stats" in skip else stats_dict(st),
            int(ns.value), int(nb.value))


def same(got, want, skip=()):
    assert got[6] == len(want[2]) and got[7] == len(want[0])
    if "stats" not in skip:
        assert got[5] == want[5]
    for i, n in enumerate(("seqs",) + OUTS[:4]):
        if n in skip:
            continue
        w = np.frombuffer(want[i] if i == 0 else want[i].tobytes(), dtype=np.uint8)
        if got[i].tobytes() != w.tobytes():
            diff = np.nonzero(got[i] != w)[0]
            raise AssertionError("%s differs at %d bytes, first at %s: %s / %s" % (n, len(diff), diff[:8], got[i][diff[:8]], w[diff[:8]]))


def compare(kc, contigs, links, reindex=True, **kw):
    dev_kw = {k: kw.pop(k) for k in ("shift", "rec_shift", "skip") if k in kw}
    want = M.scaffold(contigs, links, **kw)
    if reindex:
        index(kc, contigs)
    same(device_scaffold(kc, links, want, **dev_kw, **kw), want, dev_kw.get("skip", ()))
    return want


# ---- the model's cases ----------------------------------------------------------------------------------------------------
def test_the_models_two_contig_cases(kc):
    for gap in (7, 0, -20):
        for oa, ob in ((0, 0), (0, 1), (1, 0), (1, 1)):
            contigs, links, text = T.two_contigs(oa, ob, gap)
            want = compare(kc, contigs, links)
            assert M.strings(want) == [text]
    rng = np.random.default_rng(6)
    c = [T.rand_seq(rng, 30), T.rand_seq(rng, 50)]
    compare(kc, c, records([link(3, 0, splints=2, gap=4)]))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_models_random_graphs(kc, seed):
    contigs, rows = T.random_case(seed)
    for kw in (dict(overlap_slack=2, max_second_permille=500), dict(), dict(min_splints=2, min_spans=3, max_second_permille=1000, overlap_slack=64)):
        compare(kc, contigs, records(rows), **kw)
    compare(kc, [T.revc(c) for c in contigs], records([(r[0] ^ 1, r[1] ^ 1) + tuple(r[2:]) for r in rows]), overlap_slack=2)


def test_the_models_thresholds_choices_and_ambiguous_ends_beside_chosen_ones(kc):
    index(kc, T.CTG3)
    cases = [([link(1, 2, splints=2, gap=1)], dict(min_splints=2)), ([link(1, 2, splints=2, gap=1)], dict(min_splints=3)),
             ([link(1, 2, spans=2, gap=1)], {}), ([link(1, 2, spans=1, gap=1)], {}), ([link(1, 2, spans=1, gap=1)], dict(min_spans=1)),
             ([link(1, 2, splints=1, spans=1, gap=2, span_gap=30)], dict(min_spans=5)),
             ([link(1, 2, splints=1, spans=5, gap=2, span_gap=30)], dict(min_splints=2, min_spans=5)),
             ([link(1, 2, splints=1, spans=4, gap=2, span_gap=30)], dict(min_splints=2, min_spans=5))]
    two = [link(1, 2, splints=3, gap=1), link(1, 4, splints=1, gap=2)]
    cases += [(two, {}), (two, dict(max_second_permille=333)), (two, dict(max_second_permille=334)),
              ([link(1, 2, splints=1, spans=2, gap=1), link(1, 4, splints=2, spans=1, gap=2)], dict(max_second_permille=1000)),
              ([link(1, 4, splints=2, gap=1), link(1, 2, splints=2, gap=5)], dict(max_second_permille=1000)),
              ([link(1, 2, splints=3, gap=1), link(1, 4, spans=1, gap=2)], {}),
              ([link(1, 2, splints=2, gap=1), link(2, 5, splints=5, gap=2)], dict(max_second_permille=1000)),
              # an ambiguous end (1) and an end whose best is not mutual (4) beside a chosen edge {3, 6}
              (two + [link(3, 6, splints=4, gap=0)], {})]
    for rows, kw in cases:
        compare(kc, T.CTG3, records(rows), reindex=False, **kw)
    # means that round half up by floor division, on either side of zero
    for s, c in ((5, 2), (-5, 2), (7, 3), (-7, 3), (-1, 2), (1, 2), (-3, 2)):
        r = np.array([(1, 2, c, 0, -4, 4, 0, 0, s, 0), (2, 1, c, 0, -4, 4, 0, 0, s, 0)], dtype=M.LINK_DTYPE)
        compare(kc, T.CTG3, r, reindex=False, overlap_slack=0)
        r = np.array([(1, 2, 0, c, 0, 0, -4, 4, 0, s), (2, 1, 0, c, 0, 0, -4, 4, 0, s)], dtype=M.LINK_DTYPE)
        compare(kc, T.CTG3, r, reindex=False, overlap_slack=0)


def test_the_models_overlap_search(kc):
    for claimed, slack in [(12, 0), (13, 1), (11, 1), (17, 5), (7, 5), (18, 5), (6, 5), (13, 0)]:
        compare(kc, *T.overlap_case(12, claimed), overlap_slack=slack)
    for claimed, slack in [(76, 64), (77, 64), (12 + 64, 63)]:
        compare(kc, *T.overlap_case(12, claimed, la=200, lb=180), overlap_slack=slack)
    for spoil in (0, 11):
        assert compare(kc, *T.overlap_case(12, 12, spoil=spoil))[5]["overlaps_rejected"] == 1
    assert compare(kc, *T.overlap_case(12, 12, n_at=5), overlap_slack=3)[5]["overlaps_rejected"] == 1
    assert compare(kc, *T.overlap_case(29, 29, la=40, lb=30))[5]["edges_joined"] == 1
    compare(kc, ["ACGTTGCAGGATC", "GTTGCAGGATC"], records([link(1, 2, splints=2, gap=-11)]), overlap_slack=2)
    for claimed in (5, 9, 12):
        compare(kc, ["GGGGGGAAAAAAAA", "AAAAAAAATTTTTT"], records([link(1, 2, splints=2, gap=-claimed)]), overlap_slack=3)
    compare(kc, ["GGGGGGACACACAC", "ACACACACTTTTTT"], records([link(1, 2, splints=2, gap=-5)]), overlap_slack=3)
    # all four orientation pairs of an overlap longer than a wave, spoiled in its last byte and not
    for oa, ob in ((0, 0), (0, 1), (1, 0), (1, 1)):
        contigs, links, _ = T.two_contigs(oa, ob, -20)
        compare(kc, contigs, links)
        rng = np.random.default_rng(8)
        A = T.rand_seq(rng, 400)
        B = A[-300:] + T.rand_seq(rng, 100)
        for Bx in (B, B[:299] + ("A" if B[299] != "A" else "C") + B[300:], B[:64] + ("A" if B[64] != "A" else "C") + B[65:]):
            c = [T.revc(A) if oa else A, T.revc(Bx) if ob else Bx]
            compare(kc, c, records([link(0 if oa else 1, 3 if ob else 2, splints=3, gap=-300)]))


# ---- chains and cycles: the jump rounds, 17-bit end numbers -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, (1 << 15) + 1])
def test_chains(kc, n):
    contigs, links = T.chain_case(n, seed=n)
    want = compare(kc, contigs, links)
    assert want[5]["scaffolds"] == 1 and want[5]["edges_joined"] == n - 1 and int(want[2][0]["n_members"]) == n


@pytest.mark.parametrize("n", [2, 3, 64, 1000])
def test_cycles(kc, n):
    for seed in ((0, 1, 2, 3) if n < 64 else (n,)):
        contigs, links = T.chain_case(n, seed=seed, cycle=True)
        want = compare(kc, contigs, links)
        assert want[5]["circular"] == 1 and want[5]["scaffolds"] == 1 and int(want[2][0]["flags"]) == M.CIRCULAR
    # a cycle, a chain and singles side by side
    a, la = T.chain_case(n, seed=5, cycle=True)
    b, lb = T.chain_case(7, seed=6)
    lb = lb.copy()
    lb["from"] += 2 * (len(a) + 1)
    lb["to"] += 2 * (len(a) + 1)
    want = compare(kc, a + ["ACGT"] + b + ["", "N"], np.concatenate([la, lb]))
    assert (want[5]["circular"], want[5]["scaffolds"], want[5]["singletons"]) == (1, 5, 3)


def test_the_chain_whose_higher_end_heads_neither_path(kc):
    rng = np.random.default_rng(2)
    c = [T.rand_seq(rng, 10), T.rand_seq(rng, 12), T.rand_seq(rng, 14)]
    compare(kc, c, records([link(5, 0, splints=2, gap=1), link(1, 2, splints=2, gap=2)]))


# ---- the writer -------------------------------------------------------------------------------------------------------
WRITER_LENS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097, 70000]
WRITER_JOINS = [0, 1, 15, 16, 17, -1, -63, -64, -65, 1000, 0, -300]


@pytest.fixture(scope="module")
def writer_case():
    lens = WRITER_LENS + WRITER_LENS[::-1]
    joins = WRITER_JOINS + [-300, 1000, 1, -65, -64, -63, -1, 17, 16, 15, 1, 0]  # 70000 on 70000 first; an overlap is shorter than either text
    strands = [i % 2 for i in range(24)]  # length WRITER_LENS[j] at positions j and 23 - j: once on either strand
    rng = np.random.default_rng(4)
    order = [int(x) for x in rng.permutation(24)]
    contigs, links = T.chain_of(lens, joins, strands, order, seed=7)
    want = M.scaffold(contigs, links)
    assert want[5]["scaffolds"] == 1 and want[5]["edges_joined"] == 23
    assert {1, 15, 16, 17, 1000} <= {int(m["join"]) for m in want[3]} and {-1, -63, -64, -65, -300} <= {int(m["join"]) for m in want[3]}
    assert {(int(m["orient"]), len(contigs[int(m["ctg"])])) for m in want[3]} == {(s, n) for s in (0, 1) for n in WRITER_LENS}
    return contigs, links, want


@pytest.mark.parametrize("shift", range(16))
def test_writer_sizes_at_every_destination_alignment(kc, writer_case, shift):
    contigs, links, want = writer_case
    index(kc, contigs)
    same(device_scaffold(kc, links, want, shift=shift), want)


def test_short_members_at_every_alignment(kc):
    # members of 1 .. 40 bytes start at every position mod 16, on either strand; many members inside one 16-byte chunk
    contigs, links = T.chain_case(300, seed=12, lens=(1, 4), gaps=(0, 3))
    want = compare(kc, contigs, links)
    assert {int(m["out_pos"]) % 16 for m in want[3]} == set(range(16))
    compare(kc, contigs, links, reindex=False, shift=5)


# ---- ends and hubs -------------------------------------------------------------------------------------------------------
def test_a_hub_end_with_3000_partners(kc):
    contigs, links = T.hub_case(3000)
    want = compare(kc, contigs, links, max_second_permille=500)
    assert want[5]["ends_ambiguous"] == 1 and want[5]["ends_not_mutual"] == 2999 and want[5]["scaffolds"] == 3001
    for winner in (1, 64, 65, 2999, 3000):
        want = compare(kc, contigs, T.hub_case(3000, winner=winner)[1], reindex=False, max_second_permille=500)
        assert want[5]["edges_joined"] == 1 and int(want[3][1]["ctg"]) == winner
    # ties over the whole row: the smallest `to` wins, and the second makes the end ambiguous unless the permille is 1000
    want = compare(kc, contigs, links, reindex=False, max_second_permille=1000)
    assert want[5]["edges_joined"] == 1 and int(want[3][1]["ctg"]) == 1


# ---- degenerate inputs, optional outputs, capacity ------------------------------------------------------------------------
def test_no_links_one_contig_and_empty_contigs(kc):
    compare(kc, ["ACG", "", "T"], records([]))
    compare(kc, ["ACG", "", "T"], records([link(1, 2, splints=1, gap=2), link(3, 4, splints=1, gap=-1)]), overlap_slack=4)
    compare(kc, ["ACGTTGCA"], records([]))
    compare(kc, [""], records([]))
    compare(kc, ["", ""], records([link(1, 2, splints=1, gap=3)]))


def small_case():
    contigs, rows = T.random_case(2)
    return contigs, records(rows)


def test_each_optional_output_null_in_turn_the_size_query_and_the_capacity(kc):
    contigs, links = small_case()
    want = M.scaffold(contigs, links, overlap_slack=2)
    index(kc, contigs)
    for n in OUTS:
        same(device_scaffold(kc, links, want, skip=(n,), overlap_slack=2), want, skip=(n,))
    same(device_scaffold(kc, links, want, skip=OUTS, overlap_slack=2), want, skip=OUTS)
    counts = (len(want[2]), len(want[0]), want[5])
    assert device_scaffold(kc, links, want, query=True, overlap_slack=2) == counts
    assert device_scaffold(kc, links, want, query=True, skip=("stats",), overlap_slack=2)[:2] == counts[:2]
    for cap in (len(want[0]) - 1, 0):
        assert device_scaffold(kc, links, want, expect=_lib.KC_ERR_CAPACITY, capacity=cap, overlap_slack=2) == counts
        assert b"kc_scaffold: %d bytes, the array holds %d" % (len(want[0]), cap) in pkg.lib().kc_last_error()
    same(device_scaffold(kc, links, want, capacity=len(want[0]) + 100, overlap_slack=2), want)


def test_host_arrays_device_tensors_and_the_wrapper_twice(kc):
    import torch
    contigs, links = small_case()
    want = M.scaffold(contigs, links, overlap_slack=2)
    index(kc, contigs)
    for _ in range(2):
        seqs, offsets, scafs, members, st = kc.scaffolds(links.view(pkg.kcount.LINK_DTYPE), overlap_slack=2)
        assert (seqs.tobytes(), offsets.tobytes(), scafs.tobytes(), members.tobytes(), st) == (want[0], want[1].tobytes(), want[2].tobytes(),
                                                                                             want[3].tobytes(), want[5])
        assert scafs.dtype == pkg.kcount.SCAFFOLD_DTYPE and members.dtype == pkg.kcount.MEMBER_DTYPE
        d = torch.from_numpy(np.frombuffer(links.tobytes(), dtype=np.uint8).copy()).cuda()
        seqs, offsets, scafs, members, st = kc.scaffolds(d, overlap_slack=2)
        assert all(x.is_cuda for x in (seqs, offsets, scafs, members)) and st == want[5]
        assert (seqs.cpu().numpy().tobytes(), offsets.cpu().numpy().tobytes(), scafs.cpu().numpy().tobytes(), members.cpu().numpy().tobytes()) == (
            want[0], want[1].tobytes(), want[2].tobytes(), want[3].tobytes())
        assert kc.scaffold_strings(d, overlap_slack=2) == M.strings(want) == kc.scaffold_strings(links, overlap_slack=2)
    # host arrays through the C interface, every output
    lib = pkg.lib()
    n, ns = len(contigs), len(want[2])
    h = (np.zeros(len(want[0]), np.uint8), np.zeros(ns + 1, np.uint64), np.zeros(ns, M.SCAFFOLD_DTYPE), np.zeros(n, M.MEMBER_DTYPE), np.zeros(n, np.uint32))
    st, cs, cb = _lib.kc_scaf_stats(), C.c_uint64(0), C.c_uint64(0)
    p = _lib.kc_scaf_params(**M.params(overlap_slack=2))
    assert lib.kc_scaffold(kc._h, links.ctypes.data, len(links), 0, C.byref(p), h[0].ctypes.data, len(h[0]), h[1].ctypes.data, h[2].ctypes.data,
                           h[3].ctypes.data, h[4].ctypes.data, C.byref(cs), C.byref(cb), C.byref(st)) == 0, lib.kc_last_error()
    assert [x.tobytes() for x in h] == [want[0]] + [x.tobytes() for x in want[1:5]] and stats_dict(st) == want[5]
    # no links at all through the wrapper
    assert kc.scaffold_strings(np.zeros(0, dtype=pkg.kcount.LINK_DTYPE)) == contigs


# ---- invalid input and the order of the checks ---------------------------------------------------------------------------------
def test_invalid_records_are_named_and_nothing_is_written(kc):
    index(kc, T.CTG3)
    want = M.scaffold(T.CTG3, T.GOOD)
    same(device_scaffold(kc, T.GOOD, want), want)
    for links, bad in T.invalid_cases():
        device_scaffold(kc, links, want, expect=_lib.KC_ERR_INVALID_ARG)
        assert b"kc_scaffold: record %d is invalid" % bad in pkg.lib().kc_last_error(), (bad, pkg.lib().kc_last_error())
    two = T.spoiled(4, splint_gap_min=9)
    two[1]["to"] = 99
    device_scaffold(kc, two, want, expect=_lib.KC_ERR_INVALID_ARG)
    assert b"kc_scaffold: record 1 is invalid" in pkg.lib().kc_last_error()
    # the parameters come first, then the alignment, then the index, then the records
    device_scaffold(kc, two, want, expect=_lib.KC_ERR_INVALID_ARG, overlap_slack=65, rec_shift=8)
    assert b"overlap_slack 65 over 64" in pkg.lib().kc_last_error()
    device_scaffold(kc, two, want, expect=_lib.KC_ERR_INVALID_ARG, rec_shift=8)
    assert b"kc_scaffold: a device record array is 16-byte aligned" in pkg.lib().kc_last_error()
    same(device_scaffold(kc, T.GOOD, want), want)


def test_index_states_and_ranks():
    want = M.scaffold(T.CTG3, T.GOOD)
    with pkg.KmerCounter(K) as kc:
        device_scaffold(kc, T.GOOD, want, expect=_lib.KC_ERR_STATE)  # no index
        assert b"kc_scaffold: no contig index" in pkg.lib().kc_last_error()
        index(kc, T.CTG3)
        same(device_scaffold(kc, T.GOOD, want), want)
        kc.clear_contig_index()
        device_scaffold(kc, T.GOOD, want, expect=_lib.KC_ERR_STATE)
        index(kc, T.CTG3[:3])  # a rebuilt index with three contigs: ends 6 and 7 are gone, record 1 is (1, 6)
        device_scaffold(kc, T.GOOD, want, expect=_lib.KC_ERR_INVALID_ARG)
        assert b"kc_scaffold: record 1 is invalid" in pkg.lib().kc_last_error()
        other = [T.revc(c) for c in T.CTG3]
        index(kc, other)
        want2 = M.scaffold(other, T.GOOD)
        same(device_scaffold(kc, T.GOOD, want2), want2)
        kc.reset()
        device_scaffold(kc, T.GOOD, want, expect=_lib.KC_ERR_STATE)
    with pkg.KmerCounter(K, rank_me=1, rank_n=2) as kc:
        index(kc, T.CTG3)
        same(device_scaffold(kc, T.GOOD, want), want)


def test_names_and_launch_counts_in_the_kernel_times():
    contigs, links = T.chain_case(65, seed=3)
    with pkg.KmerCounter(K, time_kernels=True) as kc:
        index(kc, contigs)
        kc.kernel_times(clear=True)
        kc.scaffolds(links)  # a size query and the call
        t = kc.kernel_times()
    rounds = 8 + 1  # ceil(log2 130) + 1
    want = {"kc_scaf_check_kernel": 2, "kc_link_end_first_kernel<scaffold>": 2, "kc_scaf_choose_kernel": 2, "kc_scaf_edge_kernel": 2,
            "kc_scaf_next_kernel": 2, "kc_unitig_min_jump_kernel<scaffold>": 2 * rounds, "kc_unitig_cut_kernel<scaffold>": 2,
            "kc_scaf_weight_kernel": 2, "kc_unitig_rank_jump_kernel<scaffold>": 2 * rounds, "kc_unitig_rank_jump_kernel<scaffold pos>": 2 * rounds,
            "kc_scaf_select_kernel": 2, "kc_scaf_scan_kernel": 4, "kc_scaf_members_kernel": 1, "kc_scaf_records_kernel": 1, "kc_scaf_write_kernel": 1}
    assert {n: c for n, (c, _) in t.items()} == want


# ---- through the device's own steps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LC.LAYOUTS))
def test_after_the_devices_own_alignment_and_link_steps(name):
    """index_contigs -> align_reads -> align_gapped -> pair_inserts -> ctg_links -> scaffolds over tests/links_cases.py's
    construction: the result is the model's and the genome's, and index_contigs takes the scaffold block as it is"""
    layout, gaps = LC.LAYOUTS[name]
    G = LC.genome(19)
    contigs = LC.contigs_of(G, layout)
    reads, places = LC.pairs_of(G, 19)
    b, o = read_arrays(reads)
    kw = dict(insert_avg=LC.FRAGMENT, max_insert=1000, end_slack=0, max_overlap=50, max_splint_gap=50)
    with pkg.KmerCounter(LC.K) as kc:
        kc.index_contigs(*block_arrays(contigs))
        alns, first, _ = kc.align_reads(b, o)
        gapped, _ = kc.align_gapped(b, o, alns)
        hist, pairs, ist = kc.pair_inserts(o, gapped, max_insert=1000)
        links, end_first, lst, gap = kc.ctg_links(o, gapped, pairs, **kw)
        seqs, offsets, scafs, members, st = kc.scaffolds(links)
        want = M.scaffold(contigs, links.view(M.LINK_DTYPE))
        assert (seqs.tobytes(), offsets.tobytes(), scafs.tobytes(), members.tobytes(), st) == (want[0], want[1].tobytes(), want[2].tobytes(),
                                                                                             want[3].tobytes(), want[5])
        same(device_scaffold(kc, links.view(M.LINK_DTYPE), want), want)
        assert kc.scaffold_strings(links) == [T.layout_text(name, G)]
        assert T.members_of(want) == [(0, "+", 0), (1, "+", 10 if name == "gaps" else -20), (2, "-", 5)]
        # the earlier calls answer as before
        assert kc.align_reads(b, o)[0].tobytes() == alns.tobytes()
        assert kc.align_gapped(b, o, alns)[0].tobytes() == gapped.tobytes()
        assert kc.pair_inserts(o, gapped, max_insert=1000)[1].tobytes() == pairs.tobytes()
        again = kc.ctg_links(o, gapped, pairs, **kw)
        assert again[0].tobytes() == links.tobytes() and again[2] == lst
        # the scaffold block is a contig block
        info = kc.index_contigs(seqs, offsets)
        assert kc.contig_index_info() == (len(seqs), 1)
        assert kc.scaffold_strings(np.zeros(0, dtype=pkg.kcount.LINK_DTYPE)) == [T.layout_text(name, G)]
