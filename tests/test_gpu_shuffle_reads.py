"""kc_shuffle_reads (csrc/kc_shuffle.hpp) against the host model tests/shuffle_model.py, byte for byte: every output and the
statistics on the same inputs, from device arrays and from host arrays.  The model is never replaced by a second device
run.

Every call goes through `shuffle`: every array of exactly its size between canaries, the byte arrays (bases, quals and
their outputs) at any misalignment, so that source and destination spans start at every residue modulo 16.  The call
reads no contig base, so the records are forged: a read has at most one record, and the pairs name them."""
import ctypes as C

import numpy as np
import pytest

import mhm2_kmer_analysis_v2_amd as pkg
import shuffle_model as M
from depth_model import NO_ALN, PAIR_DTYPE
from mhm2_kmer_analysis_v2_amd import _lib
from test_gpu_aln_depths import PAD, lengths_index

pytestmark = pytest.mark.gpu

SORT_TILE, SCAN_TILE = 4096, 1024  # kc_sort.hpp, kc_links.hpp: pairs a workgroup and pass, reads a workgroup of the scan
MIXED = (0, 1, 15, 16, 17, 150, 1024)
SMALL = [40, 300, 1]
MANY = [30] * 5000 + [70000]  # 5001 contigs: two digits of the home field; 70 000 bases: 17 bits of anchor, three digits
OUTS = ("bases", "quals", "offsets", "order", "home", "part_starts", "gap_alns", "pairs")
UNTOUCHED = dict(dict.fromkeys(M.SHUFFLE_STATS, 0), pairs=99)


def forge(seed, ctg_lens, read_lens, frac=0.7, scores=3):
    """a case: reads of these lengths with random bytes; a read with bases has a record with probability frac, anywhere on
    a random contig, scores in [1, scores] so that ties are common; the records in random order"""
    rng = np.random.default_rng(seed)
    ctg_lens, read_lens = np.asarray(ctg_lens, dtype=np.int64), np.asarray(read_lens, dtype=np.int64)
    nreads = len(read_lens)
    offsets = np.zeros(nreads + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(read_lens)
    total = int(offsets[-1])
    bases = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=total).astype(np.uint8)
    quals = rng.integers(33, 74, size=total).astype(np.uint8)
    reads = np.nonzero((rng.random(nreads) < frac) & (read_lens > 0))[0]
    reads = reads[rng.permutation(len(reads))]
    ctg = rng.integers(0, len(ctg_lens), size=len(reads))
    span = rng.integers(1, np.minimum(read_lens[reads], ctg_lens[ctg]) + 1)
    cstart = rng.integers(0, ctg_lens[ctg] - span + 1)
    alns = np.zeros(len(reads), dtype=M.GAP_ALN_DTYPE)
    alns["read"], alns["ctg"], alns["cstart"], alns["cstop"], alns["rstop"] = reads, ctg, cstart, cstart + span, span
    alns["score"], alns["orient"], alns["seeds"] = rng.integers(1, scores + 1, size=len(reads)), rng.integers(0, 2, size=len(reads)), 1
    of_read = np.full(nreads, NO_ALN, dtype=np.uint32)
    of_read[reads] = np.arange(len(reads), dtype=np.uint32)
    pairs = np.zeros(nreads // 2, dtype=PAIR_DTYPE)
    pairs["aln0"], pairs["aln1"] = of_read[0::2], of_read[1::2]
    pairs["insert"], pairs["cls"] = rng.integers(0, 1000, size=nreads // 2), rng.integers(0, 7, size=nreads // 2)  # carried, not read
    return dict(ctg_lens=[int(x) for x in ctg_lens], bases=bases, quals=quals, offsets=offsets, alns=alns, pairs=pairs)


def model(case, parts=1, quals=True):
    return M.shuffle_reads(case["ctg_lens"], case["bases"].tobytes(), case["quals"].tobytes() if quals else None, case["offsets"], case["alns"],
                           case["pairs"], parts)


class Buf:
    """n bytes at PAD + shift of an array filled with `fill`, on the device or on the host"""

    def __init__(self, raw, n, shift, fill, dev):
        n = n if raw is None else len(raw)
        self.n, self.at, self.dev = n, PAD + shift, dev
        self.h = np.full(n + 2 * PAD + 16, fill, dtype=np.uint8)
        if raw is not None:
            self.h[self.at:self.at + n] = np.frombuffer(raw, dtype=np.uint8)
        self.image = self.h.copy()
        if dev:
            import torch
            self.t = torch.from_numpy(self.h.copy()).cuda()

    def ptr(self):
        return (self.t.data_ptr() if self.dev else self.h.ctypes.data) + self.at

    def now(self):
        return self.t.cpu().numpy() if self.dev else self.h


def stats_dict(st):
    return {n: int(getattr(st, n)) for n in M.SHUFFLE_STATS}


def shuffle(kc, case, parts=1, quals=True, dev=True, want_alns=True, want_pairs=True, want_stats=True, expect=0, shifts=(0, 0, 0, 0),
            want=None, alias=None):
    """the call; expect == 0: every output is the model's (want: the model's result where the caller has it), the canaries
    and the inputs are as they were.  expect != 0: the status, and nothing at all was written.  shifts: the misalignments
    of bases, quals, bases_out, quals_out; alias: (output, input) to pass the input's address for the output."""
    import torch
    nreads, na = len(case["offsets"]) - 1, len(case["alns"])
    npairs, total = nreads // 2, len(case["bases"])
    ins = {"bases": Buf(case["bases"].tobytes(), total, shifts[0], 0xCD, dev), "quals": Buf(case["quals"].tobytes(), total, shifts[1], 0xCD, dev),
           "offsets": Buf(case["offsets"].tobytes(), (nreads + 1) * 8, 0, 0xCD, dev), "alns": Buf(case["alns"].tobytes(), na * 32, 0, 0xCD, dev),
           "pairs": Buf(case["pairs"].tobytes(), npairs * 16, 0, 0xCD, dev)}
    sizes = {"bases": total, "quals": total, "offsets": (nreads + 1) * 8, "order": npairs * 4, "home": npairs * 4, "part_starts": (parts + 1) * 8,
             "gap_alns": na * 32, "pairs": npairs * 16}
    outs = {k: Buf(None, sizes[k], {"bases": shifts[2], "quals": shifts[3]}.get(k, 0), 0xAB, dev) for k in OUTS}
    if dev:
        torch.cuda.synchronize()
    p = {k: v.ptr() for k, v in outs.items()}
    if alias:
        p[alias[0]] = ins[alias[1]].ptr()
    st = _lib.kc_shuffle_stats(pairs=99)
    rc = pkg.lib().kc_shuffle_reads(kc._h, ins["bases"].ptr(), ins["quals"].ptr() if quals else None, ins["offsets"].ptr(), nreads,
                                    ins["alns"].ptr() if na else None, na, ins["pairs"].ptr() if npairs else None, 1 if dev else 0, parts,
                                    p["bases"], p["quals"] if quals else None, p["offsets"], p["order"], p["home"], p["part_starts"],
                                    p["gap_alns"] if want_alns else None, p["pairs"] if want_pairs else None, C.byref(st) if want_stats else None)
    for k, v in ins.items():
        assert (v.now() == v.image).all(), "the input %s was written" % k
    got = {k: v.now() for k, v in outs.items()}
    if expect:
        assert rc == expect, (rc, pkg.lib().kc_last_error())
        for k, v in got.items():
            assert (v == 0xAB).all(), "a refused call wrote %s" % k
        assert stats_dict(st) == UNTOUCHED, "a refused call wrote the statistics"
        return rc
    assert rc == 0, pkg.lib().kc_last_error()
    want = want or model(case, parts, quals)
    wanted = dict(quals=quals, gap_alns=want_alns, pairs=want_pairs)
    for k, buf in outs.items():
        g = got[k]
        assert (g[:buf.at] == 0xAB).all() and (g[buf.at + buf.n:] == 0xAB).all(), "a canary of %s was written" % k
        body = g[buf.at:buf.at + buf.n]
        if not wanted.get(k, True):
            assert (body == 0xAB).all(), "%s was written though it was not asked for" % k
            continue
        w = np.frombuffer(want[k], dtype=np.uint8)
        assert len(w) == buf.n, (k, len(w), buf.n)
        if body.tobytes() != want[k]:
            diff = np.nonzero(body != w)[0]
            raise AssertionError("%s differs at bytes %s of %d: got %s, want %s" % (k, diff[:8], buf.n, body[diff[:8]], w[diff[:8]]))
    assert stats_dict(st) == (want["stats"] if want_stats else UNTOUCHED)
    return want


@pytest.fixture(scope="module")
def small():
    with lengths_index(SMALL, time_kernels=True) as kc:
        yield kc


@pytest.fixture(scope="module")
def many():
    with lengths_index(MANY) as kc:
        yield kc


# ---- sizes and shapes ---------------------------------------------------------------------------------------------------
def test_no_pairs_and_one_pair(small):
    empty = forge(1, SMALL, [])
    for dev in (True, False):
        for parts in (1, 5):
            w = shuffle(small, empty, parts=parts, dev=dev)
            assert w["offsets"] == bytes(8) and w["part_starts"] == bytes(8 * (parts + 1)) and w["stats"]["pairs"] == 0
        shuffle(small, empty, quals=False, want_alns=False, want_pairs=False, dev=dev)
    for seed, lens, frac in ((2, [17, 150], 1.0), (3, [0, 0], 1.0), (4, [1, 0], 1.0), (5, [150, 16], 0.0), (6, [1024, 1024], 1.0)):
        one = forge(seed, SMALL, lens, frac=frac)
        for dev in (True, False):
            for parts in (1, 2):
                w = shuffle(small, one, parts=parts, dev=dev, shifts=(3, 5, 7, 9))
                assert w["order"] == bytes(4) and w["stats"]["homed"] == (1 if frac and sum(lens) else 0)


@pytest.mark.parametrize("shifts", [(0, 0, 0, 0), (1, 15, 0, 0), (0, 0, 15, 1), (5, 9, 13, 2), (8, 8, 8, 8)])
def test_mixed_read_lengths_at_every_residue(small, shifts):
    """300 pairs whose reads have 0, 1, 15, 16, 17, 150 or 1024 bases: pairs shorter than a 16-byte chunk, chunks that
    span several pairs (empty ones among them), long runs inside one pair; the arrays themselves at odd addresses"""
    rng = np.random.default_rng(sum(shifts))
    lens = [MIXED[i] for i in rng.integers(0, len(MIXED), size=600)]
    case = forge(7 + sum(shifts), SMALL, lens)
    w = shuffle(small, case, parts=3, shifts=shifts)
    assert w["stats"]["homed"] > 100 and w["stats"]["homeless"] > 20 and w["stats"]["homes"] == 3
    noff, order = np.frombuffer(w["offsets"], dtype=np.uint64), np.frombuffer(w["order"], dtype=np.uint32)
    # (where a pair's bytes lay, where they lie now) modulo 16, the arrays' own misalignments included
    residues = {((int(case["offsets"][2 * int(p)]) + shifts[0]) % 16, (int(noff[2 * q]) + shifts[2]) % 16) for q, p in enumerate(order)}
    assert len(residues) > 100 and len({a for a, _ in residues}) == len({b for _, b in residues}) == 16
    if shifts == (5, 9, 13, 2):
        shuffle(small, case, parts=3, shifts=shifts, dev=False, want=w)


def test_short_reads_only(small):
    """every read 0, 1 or 2 bases: every chunk spans many pairs"""
    rng = np.random.default_rng(11)
    case = forge(11, SMALL, rng.integers(0, 3, size=2000))
    shuffle(small, case, parts=2, shifts=(1, 2, 3, 4))
    w = model(case, 2, False)
    shuffle(small, case, parts=2, quals=False, shifts=(1, 2, 3, 4), want=w)
    shuffle(small, case, parts=2, quals=False, dev=False, want=w)


def test_optional_outputs_in_turn(small):
    case = forge(12, SMALL, [150, 30, 151, 1, 17, 0] * 20)
    for quals in (True, False):
        w = model(case, 2, quals)
        for dev in (True, False):
            for want_alns, want_pairs in ((True, True), (False, True), (True, False), (False, False)):
                shuffle(small, case, parts=2, quals=quals, dev=dev, want_alns=want_alns, want_pairs=want_pairs, want=w)
            shuffle(small, case, parts=2, quals=quals, dev=dev, want_stats=False, want=w)
    # no records at all: every pair is homeless, the order is the old one
    none = dict(case, alns=case["alns"][:0], pairs=case["pairs"].copy())
    none["pairs"]["aln0"] = none["pairs"]["aln1"] = NO_ALN
    w = shuffle(small, none, parts=2)
    assert np.frombuffer(w["order"], dtype=np.uint32).tolist() == list(range(60)) and w["bases"] == case["bases"].tobytes()


@pytest.mark.parametrize("parts", [1, 2, 7, 65536])
def test_parts(small, parts):
    rng = np.random.default_rng(13)
    case = forge(13, SMALL, rng.integers(30, 152, size=6000))
    w = shuffle(small, case, parts=parts, shifts=(0, 4, 8, 12))
    starts = np.frombuffer(w["part_starts"], dtype=np.uint64)
    assert len(starts) == parts + 1 and int(starts[-1]) == 3000 and (np.diff(starts.astype(np.int64)) >= 0).all()
    if parts == 7:
        shuffle(small, case, parts=parts, dev=False, want=w)


def test_all_homeless_and_all_homed(small):
    rng = np.random.default_rng(14)
    lens = rng.integers(30, 152, size=5000)
    w = shuffle(small, forge(14, SMALL, lens, frac=0.0), parts=3)
    assert (w["stats"]["homed"], w["stats"]["homeless"], w["stats"]["homes"], w["stats"]["max_home_pairs"]) == (0, 2500, 0, 0)
    w = shuffle(small, forge(15, SMALL, lens, frac=1.0), parts=3)
    assert (w["stats"]["homed"], w["stats"]["homeless"], w["stats"]["one_mate"]) == (2500, 0, 0)


def test_one_contig():
    """one contig of 40 bases: a home field of one bit, runs of equal keys longer than a sort tile is wide"""
    rng = np.random.default_rng(16)
    case = forge(16, [40], rng.integers(30, 152, size=2 * SORT_TILE + 2 * 77), frac=0.9, scores=2)
    with lengths_index([40]) as kc:
        w = shuffle(kc, case, parts=2)
        assert w["stats"]["homes"] == 1 and w["stats"]["max_home_pairs"] == w["stats"]["homed"] > SORT_TILE - 200
        assert w["stats"]["key_bits"] == 6 + 1


def test_many_contigs_and_a_long_one(many):
    """5001 contigs, one of 70 000 bases: key_bits = 17 + 13, four radix passes, the last over six bits"""
    rng = np.random.default_rng(17)
    case = forge(17, MANY, rng.integers(30, 152, size=12000), frac=0.8)
    # anchors on the long contig that need the third digit, beside the short contigs' below 30
    at = np.nonzero((case["alns"]["read"] % 7 == 0) & (case["alns"]["cstop"] - case["alns"]["cstart"] < 100))[0]
    span = case["alns"]["cstop"][at] - case["alns"]["cstart"][at]
    case["alns"]["ctg"][at] = 5000
    case["alns"]["cstart"][at] = 65536 + rng.integers(0, 4000, size=len(at))
    case["alns"]["cstop"][at] = case["alns"]["cstart"][at] + span
    w = shuffle(many, case, parts=7)
    assert w["stats"]["key_bits"] == 30 and w["stats"]["homes"] > 2000
    home = np.frombuffer(w["home"], dtype=np.uint32)
    assert (home == 5000).sum() > 100
    shuffle(many, case, parts=7, dev=False, want=w)


@pytest.fixture(scope="module")
def forty_thousand():
    rng = np.random.default_rng(18)
    case = forge(18, SMALL, rng.integers(30, 152, size=80000))
    return case, model(case, 7, True)


@pytest.mark.parametrize("dev", [True, False])
def test_forty_thousand_pairs(small, forty_thousand, dev):
    """more than one sort tile (ten) and more than one scan tile (seventy-nine)"""
    case, w = forty_thousand
    assert len(case["pairs"]) > 2 * SORT_TILE and len(case["offsets"]) > 2 * SCAN_TILE
    shuffle(small, case, parts=7, dev=dev, shifts=(0, 0, 0, 0) if not dev else (2, 11, 6, 15), want=w)


# ---- the protocol -------------------------------------------------------------------------------------------------------
def expected_launches(case, want_remap=True):
    nreads, na, bits = len(case["offsets"]) - 1, len(case["alns"]), M.key_bits(case["ctg_lens"], (len(case["offsets"]) - 1) // 2)
    passes = (bits + 7) // 8
    want = {"kc_shuf_offsets_kernel": 1, "kc_shuf_parts_kernel": 1}
    if nreads:
        want.update({"kc_align_lengths_kernel<shuffle>": 1, "kc_lassm_pair_check_kernel<shuffle>": 1, "kc_shuf_longest_kernel": 1,
                     "kc_shuf_key_kernel": 1, "kc_sort_hist_kernel<shuffle>": passes, "kc_sort_scan_kernel<shuffle>": passes,
                     "kc_sort_scatter_kernel<shuffle>": passes, "kc_shuf_place_kernel": 1, "kc_link_tile_scan_kernel<shuffle>": 1,
                     "kc_shuf_scan_kernel": 1})
    if na:
        want["kc_depth_check_kernel<shuffle>"] = 1
    if len(case["bases"]):
        want["kc_shuf_gather_kernel"] = 1
    if want_remap and (na or nreads):
        want["kc_shuf_remap_kernel"] = 1
    return want


def test_names_and_launch_counts_in_the_kernel_times(small):
    case = forge(19, SMALL, [150, 30] * 50)
    assert M.key_bits(SMALL, 50) == 9 + 2
    for kw, remap in ((dict(), True), (dict(want_alns=False, want_pairs=False), False), (dict(quals=False), True)):
        small.kernel_times(clear=True)
        shuffle(small, case, parts=2, **kw)
        assert {n: c for n, (c, _) in small.kernel_times(clear=True).items()} == expected_launches(case, remap)
    empty = forge(1, SMALL, [])
    shuffle(small, empty)
    assert {n: c for n, (c, _) in small.kernel_times(clear=True).items()} == expected_launches(empty)


def test_the_wrapper_both_modes(small):
    import torch
    case = forge(20, SMALL, [150, 30, 0, 17] * 40)
    for parts, quals, remap in ((1, True, True), (3, False, True), (3, True, False)):
        w = model(case, parts, quals)
        for rep in range(2):
            out = small.shuffle_reads(case["bases"], case["quals"] if quals else None, case["offsets"], case["alns"], case["pairs"], parts=parts,
                                      remap=remap)
            assert sorted(out) == sorted(OUTS + ("stats",))
            assert out["order"].dtype == np.uint32 and out["offsets"].dtype == np.uint64
            for k in OUTS:
                if (k == "quals" and not quals) or (k in ("gap_alns", "pairs") and not remap):
                    assert out[k] is None
                else:
                    assert out[k].tobytes() == w[k], k
            assert out["stats"] == w["stats"]
        d = {k: torch.from_numpy(np.frombuffer(case[k].tobytes(), dtype=np.uint8).copy()).cuda() for k in ("bases", "quals", "alns", "pairs")}
        d_offs = torch.from_numpy(case["offsets"].view(np.int64)).cuda()
        out = small.shuffle_reads(d["bases"], d["quals"] if quals else None, d_offs, d["alns"], d["pairs"], parts=parts, remap=remap)
        for k in OUTS:
            if (k == "quals" and not quals) or (k in ("gap_alns", "pairs") and not remap):
                assert out[k] is None
            else:
                assert out[k].is_cuda and out[k].cpu().numpy().tobytes() == w[k], k
        assert out["stats"] == w["stats"]


def test_invalid_reads_records_and_pairs_are_named_and_nothing_is_written(small):
    lib = pkg.lib()
    case = forge(21, SMALL, [150, 30, 17, 16, 100, 100, 64, 64], frac=1.0)
    shuffle(small, case)
    for dev in (True, False):
        # a read over the limit, and offsets that decrease: the lowest is named
        long_case = forge(21, SMALL, [150, 30, 17, 1025, 100, 100, 1200, 64], frac=0.0)
        with pytest.raises(M.BadRead) as e:
            model(long_case)
        assert e.value.index == 3
        shuffle(small, long_case, dev=dev, expect=_lib.KC_ERR_INVALID_ARG)
        assert b"kc_shuffle_reads: read 3 is longer than 1024 bases, or its offsets decrease" in lib.kc_last_error()
        back = dict(case, offsets=case["offsets"].copy())
        back["offsets"][6] = 100
        with pytest.raises(M.BadRead) as e:
            model(back)
        assert e.value.index == 5
        shuffle(small, back, dev=dev, expect=_lib.KC_ERR_INVALID_ARG)
        assert b"kc_shuffle_reads: read 5 " in lib.kc_last_error()
        # records
        for field, value in (("ctg", 3), ("read", 8), ("orient", 2), ("kind", 3), ("cstop", 301), ("rstop", 1025)):
            bad = dict(case, alns=case["alns"].copy())
            i = 3
            bad["alns"][field][i] = value
            with pytest.raises(M.BadRecord) as e:
                model(bad)
            assert e.value.index == i
            shuffle(small, bad, dev=dev, expect=_lib.KC_ERR_INVALID_ARG)
            assert b"kc_shuffle_reads: record %d is not a valid kc_gap_aln" % i in lib.kc_last_error(), (field, lib.kc_last_error())
        # pairs: an index out of range, a record of another read, a record of kind NONE
        for p, name, value in ((1, "aln0", 8), (3, "aln1", int(case["pairs"]["aln0"][3])), (2, "aln0", 0xFFFFFFFE)):
            bad = dict(case, pairs=case["pairs"].copy())
            bad["pairs"][name][p] = value
            with pytest.raises(M.BadPair) as e:
                model(bad)
            assert e.value.index == p
            shuffle(small, bad, dev=dev, expect=_lib.KC_ERR_INVALID_ARG)
            assert b"kc_shuffle_reads: pair %d names a record" % p in lib.kc_last_error()
        none = dict(case, alns=case["alns"].copy())
        i = int(case["pairs"]["aln1"][2])
        none["alns"]["kind"][i] = M.KIND_NONE
        with pytest.raises(M.BadPair) as e:
            model(none)
        assert e.value.index == 2
        shuffle(small, none, dev=dev, expect=_lib.KC_ERR_INVALID_ARG)
        assert b"kc_shuffle_reads: pair 2 " in lib.kc_last_error()
        # with a context too: an output that is an input, an odd number of reads, parts out of range
        for alias in (("bases", "bases"), ("quals", "quals"), ("offsets", "offsets"), ("gap_alns", "alns"), ("pairs", "pairs")):
            shuffle(small, case, dev=dev, alias=alias, expect=_lib.KC_ERR_INVALID_ARG)
            assert b"the call does not work in place" in lib.kc_last_error()
        shuffle(small, case, dev=dev, parts=65537, expect=_lib.KC_ERR_INVALID_ARG)
        assert b"parts 65537 outside" in lib.kc_last_error()
        shuffle(small, case, dev=dev)
    odd = dict(case, offsets=case["offsets"][:-1])
    shuffle(small, odd, expect=_lib.KC_ERR_INVALID_ARG)
    assert b"7 reads are no pairs" in lib.kc_last_error()


def test_index_states_and_ranks():
    case = forge(22, SMALL, [150, 30, 17, 16] * 10)
    with pkg.KmerCounter(21) as kc:
        shuffle(kc, case, expect=_lib.KC_ERR_STATE)  # no index
        assert b"kc_shuffle_reads: no contig index" in pkg.lib().kc_last_error()
        shuffle(kc, case, dev=False, expect=_lib.KC_ERR_STATE)
    with lengths_index(SMALL) as kc:
        want = shuffle(kc, case, parts=2)
        kc.clear_contig_index()
        shuffle(kc, case, parts=2, expect=_lib.KC_ERR_STATE)
    with lengths_index(SMALL, rank_me=1, rank_n=2) as kc:
        shuffle(kc, case, parts=2, want=want)
