"""What kcount.py's contig-pass wrappers promise by themselves, whatever the library computes: the type, dtype and length of
every array they return for host arrays and for device tensors (and that both hold the same bytes), the keys of every
statistics dict, and the ValueErrors they raise before the library is called -- records of the wrong item size or not
contiguous, counts that do not fit, one input on the other side.  One chain over the smallest input that has links, a
scaffold and gaps to close: index_contigs -> align_reads -> align_gapped -> pair_inserts -> aln_depths -> local_assm ->
ctg_links -> scaffolds -> close_gaps -> shuffle_reads.  What the records hold is the business of the files beside this one."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import mhm2_kmer_analysis_v2_amd as pkg
from align_model import revcomp
from mhm2_kmer_analysis_v2_amd import _lib
from mhm2_kmer_analysis_v2_amd import kcount as KC
from test_gpu_gap_align import block_arrays, read_arrays

pytestmark = pytest.mark.gpu

K = 15
PARTS = 2
MAX_INSERT = 1000
KW = dict(end_slack=0, max_overlap=50, max_splint_gap=50)
LINKS_KW = dict(insert_avg=100, max_insert=MAX_INSERT, **KW)
LASSM_KW = dict(min_mer_len=7, max_walk_len=60, max_insert=300)
U8, U16, U32, U64 = np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.uint32), np.dtype(np.uint64)
TORCH_OF = {U8: "uint8", U16: "int16", U32: "int32", U64: "int64"}  # the tensor that holds the bits of a host dtype


def the_case():
    """Three 60-base contigs two bases apart in a 190-base genome (the third reversed) and a fourth from elsewhere; four
    pairs of 40-base reads: two whose reads lie across the two gaps, one that spans each gap."""
    rng = np.random.default_rng(7)
    G = "".join("ACGT"[i] for i in rng.integers(0, 4, size=190))
    other = "".join("ACGT"[i] for i in rng.integers(0, 4, size=60))
    contigs = [G[0:60], G[62:122], revcomp(G[124:184]), other]

    def pair(a, b):
        return [G[a:a + 40], revcomp(G[b:b + 40])]

    return G, contigs, pair(40, 100) + pair(43, 103)[::-1] + pair(5, 70) + pair(66, 140)


def to_device(a):
    """a host array as the wrappers take it on the device: 64-bit integers as int64, everything else as its bytes"""
    import torch
    if a is None:
        return None
    return torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.int64 if a.dtype == U64 else np.uint8).copy()).cuda()


def raw(a):
    """the bytes of a host array or of a device tensor"""
    return (a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


def walk(kc, block, b, q, o, keep_records=True):
    """the chain with every step's arrays going into the next, as the step returned them"""
    r = {"index_contigs": (kc.index_contigs(*block),)}
    alns, _, _ = r["align_reads"] = kc.align_reads(b, o)
    gapped, _ = r["align_gapped"] = kc.align_gapped(b, o, alns if keep_records else alns[:0])
    _, pairs, _ = r["pair_inserts"] = kc.pair_inserts(o, gapped, max_insert=MAX_INSERT)
    _, ctgs, _ = r["aln_depths"] = kc.aln_depths(gapped)
    r["local_assm"] = kc.local_assm(b, q, o, gapped, pairs, ctgs, **LASSM_KW)
    links, _, _, _ = r["ctg_links"] = kc.ctg_links(o, gapped, pairs, **LINKS_KW)
    _, _, scafs, members, _ = r["scaffolds"] = kc.scaffolds(links)
    r["close_gaps"] = kc.close_gaps(b, o, gapped, scafs, members, **KW)
    r["shuffle_reads"] = kc.shuffle_reads(b, q, o, gapped, pairs, parts=PARTS)
    return r


def sizes(kc, o, host):
    nbytes, n_ctgs = kc.contig_index_info()
    return SimpleNamespace(reads=len(o) - 1, pairs=(len(o) - 1) // 2, bases=int(o[-1]), block=nbytes, ctgs=n_ctgs,
                           alns=len(host["align_reads"][0]), recs=len(host["align_gapped"][0]), links=len(host["ctg_links"][0]),
                           scafs=len(host["scaffolds"][2]), lassm_bytes=len(host["local_assm"][0]),
                           scaf_bytes=len(host["scaffolds"][0]), closed_bytes=len(host["close_gaps"][0]))


def arrays_of(n):
    """every returned array of every wrapper: (place in the result, host dtype, length)"""
    return {"index_contigs": [],
            "align_reads": [(0, KC.ALN_DTYPE, n.alns), (1, U64, n.reads + 1)],
            "align_gapped": [(0, KC.GAP_ALN_DTYPE, n.recs)],
            "pair_inserts": [(0, U64, MAX_INSERT + 1), (1, KC.PAIR_DTYPE, n.pairs)],
            "aln_depths": [(0, U16, n.block), (1, KC.CTG_DEPTH_DTYPE, n.ctgs)],
            "local_assm": [(0, U8, n.lassm_bytes), (1, U64, n.ctgs + 1), (2, KC.LASSM_END_DTYPE, 2 * n.ctgs)],
            "ctg_links": [(0, KC.LINK_DTYPE, n.links), (1, U64, 2 * n.ctgs + 1)],
            "scaffolds": [(0, U8, n.scaf_bytes), (1, U64, n.scafs + 1), (2, KC.SCAFFOLD_DTYPE, n.scafs), (3, KC.MEMBER_DTYPE, n.ctgs)],
            "close_gaps": [(0, U8, n.closed_bytes), (1, U64, n.scafs + 1), (2, KC.SCAFFOLD_DTYPE, n.scafs), (3, KC.MEMBER_DTYPE, n.ctgs),
                           (4, KC.CLOSURE_DTYPE, n.ctgs)],
            "shuffle_reads": [("bases", U8, n.bases), ("quals", U8, n.bases), ("offsets", U64, n.reads + 1), ("order", U32, n.pairs),
                              ("home", U32, n.pairs), ("part_starts", U64, PARTS + 1), ("gap_alns", KC.GAP_ALN_DTYPE, n.recs),
                              ("pairs", KC.PAIR_DTYPE, n.pairs)]}


def fields(struct, *more):
    return {f for f, _ in struct._fields_ if f != "reserved"} | set(more)


# the statistics of every wrapper: (place in the result, the exact keys, the keys that hold lists)
STATS_OF = {"index_contigs": (0, fields(_lib.kc_ctg_index_stats), ()),
            "align_reads": (2, fields(_lib.kc_align_stats), ()),
            "align_gapped": (1, fields(_lib.kc_gap_stats), ()),
            "pair_inserts": (2, fields(_lib.kc_insert_stats, "mean", "stddev"), ("cls",)),
            "aln_depths": (2, fields(_lib.kc_depth_stats), ()),
            "local_assm": (3, fields(_lib.kc_lassm_stats), ("status",)),
            "ctg_links": (2, fields(_lib.kc_link_stats), ()),
            "scaffolds": (4, fields(_lib.kc_scaf_stats), ()),
            "close_gaps": (5, fields(_lib.kc_close_stats), ()),
            "shuffle_reads": ("stats", fields(_lib.kc_shuffle_stats), ())}


def check_array(h, d, dtype, count, what):
    """a returned array on the host and on the device: the types, the dtypes, the lengths, the same bytes"""
    import torch
    assert type(h) is np.ndarray and h.dtype == dtype and h.shape == (count,), what
    want = torch.uint8 if dtype.fields else getattr(torch, TORCH_OF[dtype])
    assert type(d) is torch.Tensor and d.is_cuda and d.dtype == want, what
    assert tuple(d.shape) == (count * (dtype.itemsize if dtype.fields else 1),), what
    assert d.cpu().numpy().tobytes() == h.tobytes(), what


def check_contract(host, dev, n):
    """host, dev: {wrapper: its result} of the same calls on either side, for all the wrappers or for some"""
    assert sorted(host) == sorted(dev)
    for name, arrays in arrays_of(n).items():
        if name not in host:
            continue
        for at, dtype, count in arrays:
            check_array(host[name][at], dev[name][at], dtype, count, "%s[%r]" % (name, at))
        at, keys, lists = STATS_OF[name]
        for st in (host[name][at], dev[name][at]):
            assert type(st) is dict and set(st) == keys, name
            for key, v in st.items():
                if key in lists:
                    assert type(v) is list and v and all(type(x) is int for x in v), (name, key)
                else:
                    assert type(v) is (float if key in ("mean", "stddev") else int), (name, key)
        assert host[name][at] == dev[name][at], name
    for r in (host, dev):  # ctg_links' gap column is a host array on either side
        gap = r["ctg_links"][3]
        assert type(gap) is np.ndarray and gap.dtype == np.float64 and gap.shape == (n.links,)
    assert (host["ctg_links"][3] == dev["ctg_links"][3]).all()
    assert len(host["shuffle_reads"]) == len(dev["shuffle_reads"]) == 9


@pytest.fixture(scope="module")
def chain():
    """the counter after the chain on both sides: the inputs and every step's result, as host arrays and as device tensors"""
    G, contigs, reads = the_case()
    b, o = read_arrays(reads)
    q = np.random.default_rng(8).integers(35, 74, size=len(b)).astype(np.uint8)
    block = block_arrays(contigs)
    with pkg.KmerCounter(K, time_kernels=True) as kc:
        host = walk(kc, block, b, q, o)
        d_in = [to_device(x) for x in (b, q, o)]
        dev = walk(kc, tuple(to_device(x) for x in block), *d_in)
        yield SimpleNamespace(kc=kc, G=G, contigs=contigs, block=block, b=b, q=q, o=o, d_b=d_in[0], d_q=d_in[1], d_o=d_in[2], host=host,
                              dev=dev)


def test_what_every_wrapper_returns_on_either_side(chain):
    c = chain
    n = sizes(c.kc, c.o, c.host)
    # the input is what it was made to be: records for every read, links across both gaps, two scaffolds, both gaps closed
    assert (n.reads, n.ctgs, n.links, n.scafs) == (8, 4, 4, 2) and n.recs == n.alns == 12
    assert c.host["close_gaps"][0].tobytes().decode() == c.G[:184] + "_" + c.contigs[3] + "_" and c.host["close_gaps"][5]["filled"] == 2
    check_contract(c.host, c.dev, n)
    st = c.host["pair_inserts"][2]
    assert st["cls"][_lib.KC_PAIR_PROPER] == 1 and st["mean"] == 100.0 and st["stddev"] == 0.0
    # without quals and without remap: None in their places, on either side
    for b, o, gapped, pairs in ((c.b, c.o, c.host["align_gapped"][0], c.host["pair_inserts"][1]),
                                (c.d_b, c.d_o, c.dev["align_gapped"][0], c.dev["pair_inserts"][1])):
        s = c.kc.shuffle_reads(b, None, o, gapped, pairs, parts=PARTS, remap=False)
        assert s["quals"] is None and s["gap_alns"] is None and s["pairs"] is None and len(s) == 9
        assert raw(s["bases"]) == c.host["shuffle_reads"]["bases"].tobytes()


def zero_read_calls(c, host=True):
    """the wrappers that take reads, called with none at all on one side -- as calls_of gives them; the scaffolds, members
    and contig depths are the chain's of that side"""
    side, r = ((lambda x: x), c.host) if host else (to_device, c.dev)
    b, o = side(np.zeros(0, dtype=U8)), side(np.zeros(1, dtype=U64))
    alns, gapped, pairs = (side(np.zeros(0, dtype=t)) for t in (KC.ALN_DTYPE, KC.GAP_ALN_DTYPE, KC.PAIR_DTYPE))
    ctgs, scafs, members = r["aln_depths"][1], r["scaffolds"][2], r["scaffolds"][3]
    return [("align_reads", ("bases", "offsets"), (b, o), {}),
            ("align_gapped", ("bases", "offsets", "alns"), (b, o, alns), {}),
            ("pair_inserts", ("offsets", "gap_alns"), (o, gapped), dict(max_insert=MAX_INSERT)),
            ("local_assm", ("bases", "quals", "offsets", "gap_alns", "pairs", "ctg_depths"), (b, b, o, gapped, pairs, ctgs), LASSM_KW),
            ("ctg_links", ("offsets", "gap_alns", "pairs"), (o, gapped, pairs), LINKS_KW),
            ("close_gaps", ("bases", "offsets", "gap_alns", "scaffolds", "members"), (b, o, gapped, scafs, members), KW),
            ("shuffle_reads", ("bases", "quals", "offsets", "gap_alns", "pairs"), (b, b, o, gapped, pairs), dict(parts=PARTS))]


@pytest.mark.parametrize("empty", ["records", "reads"])
def test_empty_inputs_give_arrays_of_length_zero_of_the_same_types(chain, empty):
    c = chain
    if empty == "records":  # the reads, and none of them aligned
        host = walk(c.kc, c.block, c.b, c.q, c.o, keep_records=False)
        dev = walk(c.kc, tuple(to_device(x) for x in c.block), c.d_b, c.d_q, c.d_o, keep_records=False)
        n = sizes(c.kc, c.o, host)
        assert (n.recs, n.links, n.scafs, n.pairs) == (0, 0, 4, 4)
        check_contract(host, dev, n)
        return
    # no reads at all, in every step that takes reads
    host, dev = ({m: getattr(c.kc, m)(*args, **kw) for m, _, args, kw in zero_read_calls(c, side)} for side in (True, False))
    assert sorted(host) == sorted(m for m in STATS_OF if m not in ("index_contigs", "aln_depths", "scaffolds"))
    n = SimpleNamespace(reads=0, pairs=0, bases=0, alns=0, recs=0, links=0, block=len(c.block[0]), ctgs=4, scafs=2,
                        lassm_bytes=len(c.block[0]), scaf_bytes=None, closed_bytes=len(c.host["scaffolds"][0]))
    check_contract(host, dev, n)
    assert host["local_assm"][0].tobytes() == c.block[0].tobytes()  # nothing to extend the contigs with,
    assert host["close_gaps"][0].tobytes() == c.host["scaffolds"][0].tobytes()  # and nothing to close the gaps with
    assert host["align_reads"][2]["reads"] == host["pair_inserts"][2]["pairs"] == host["shuffle_reads"]["stats"]["pairs"] == 0
    # shuffle_reads without quals or without remap: None in their places, everything else as before
    _, _, (b, _, o, gapped, pairs), _ = zero_read_calls(c)[-1]
    for quals in (b, None):
        for remap in (True, False):
            hs = c.kc.shuffle_reads(b, quals, o, gapped, pairs, parts=PARTS, remap=remap)
            ds = c.kc.shuffle_reads(*(to_device(x) for x in (b, quals, o, gapped, pairs)), parts=PARTS, remap=remap)
            for key, dtype, count in arrays_of(n)["shuffle_reads"]:
                if (key == "quals" and quals is None) or (key in ("gap_alns", "pairs") and not remap):
                    assert hs[key] is None and ds[key] is None, key
                else:
                    check_array(hs[key], ds[key], dtype, count, key)
            assert hs["stats"] == ds["stats"] == host["shuffle_reads"]["stats"] and len(hs) == len(ds) == 9


def calls_of(c, host=True):
    """every wrapper of the chain that takes arrays, as (method, names of the array arguments, the arguments, keywords) on
    one side, with the other steps' results of that side"""
    r = c.host if host else c.dev
    b, q, o = (c.b, c.q, c.o) if host else (c.d_b, c.d_q, c.d_o)
    block = c.block if host else tuple(to_device(x) for x in c.block)
    alns, gapped, pairs, ctgs = r["align_reads"][0], r["align_gapped"][0], r["pair_inserts"][1], r["aln_depths"][1]
    links, scafs, members = r["ctg_links"][0], r["scaffolds"][2], r["scaffolds"][3]
    return [("index_contigs", ("seqs", "offsets"), block, {}),
            ("align_reads", ("bases", "offsets"), (b, o), {}),
            ("align_gapped", ("bases", "offsets", "alns"), (b, o, alns), {}),
            ("aln_depths", ("gap_alns",), (gapped,), {}),
            ("pair_inserts", ("offsets", "gap_alns"), (o, gapped), dict(max_insert=MAX_INSERT)),
            ("local_assm", ("bases", "quals", "offsets", "gap_alns", "pairs", "ctg_depths"), (b, q, o, gapped, pairs, ctgs), LASSM_KW),
            ("ctg_links", ("offsets", "gap_alns", "pairs"), (o, gapped, pairs), LINKS_KW),
            ("scaffolds", ("links",), (links,), {}),
            ("close_gaps", ("bases", "offsets", "gap_alns", "scaffolds", "members"), (b, o, gapped, scafs, members), KW),
            ("shuffle_reads", ("bases", "quals", "offsets", "gap_alns", "pairs"), (b, q, o, gapped, pairs), dict(parts=PARTS))]


def refused(c, name, method, args, kw):
    """a ValueError that names the argument among those in front of its colon, raised before the library was called: its
    last error is what it was"""
    before = pkg.lib().kc_last_error()
    with pytest.raises(ValueError, match=r"^([\w, ]*\b)?%s\b[\w, ]*:" % name):
        getattr(c.kc, method)(*args, **kw)
    assert pkg.lib().kc_last_error() == before, (method, name)


def swapped(args, i, new):
    return tuple(new if j == i else a for j, a in enumerate(args))


def test_host_records_of_the_wrong_item_size_or_not_contiguous_are_refused(chain):
    c = chain
    for method, names, args, kw in calls_of(c):
        for i, name in enumerate(names):
            a = args[i]
            if a.dtype.fields is None:
                continue
            assert len(a) > 1 and a.flags["C_CONTIGUOUS"], name
            refused(c, name, method, swapped(args, i, np.zeros(len(a), dtype=np.uint8)), kw)
            strided = np.repeat(a, 2)[::2]
            assert strided.tobytes() == a.tobytes() and not strided.flags["C_CONTIGUOUS"]
            if (method, name) == ("local_assm", "ctg_depths"):
                # the one record array whose contiguity is not looked at: the call goes through, with whatever lies
                # behind the first record in memory
                seqs, offs, ends, st = c.kc.local_assm(*swapped(args, i, strided), **kw)
                assert seqs.dtype == U8 and offs.shape == (5,) and ends.shape == (8,)
                continue
            refused(c, name, method, swapped(args, i, strided), kw)


def test_counts_that_do_not_fit_are_refused(chain):
    import torch
    c = chain
    for host in (True, False):
        calls = {m: (names, args, kw) for m, names, args, kw in calls_of(c, host)}
        for method, name, size in (("local_assm", "pairs", 16), ("ctg_links", "pairs", 16), ("shuffle_reads", "pairs", 16),
                                   ("local_assm", "ctg_depths", 32), ("close_gaps", "members", 16), ("shuffle_reads", "quals", 1)):
            names, args, kw = calls[method]
            i = names.index(name)
            one = args[i][:1 if host else size]  # a record less, and a record more
            refused(c, name, method, swapped(args, i, args[i][:-len(one)]), kw)
            refused(c, name, method, swapped(args, i, np.concatenate([args[i], one]) if host else torch.cat([args[i], one])), kw)


def test_one_input_on_the_other_side_is_refused(chain):
    c = chain
    for host in (True, False):
        here, there = calls_of(c, host), calls_of(c, not host)
        for (method, names, args, kw), (_, _, others, _) in zip(here, there):
            if len(names) < 2:
                continue
            for i, name in enumerate(names):
                refused(c, name, method, swapped(args, i, others[i]), kw)
        # close_gaps looks at its offsets, scaffolds and members even when they are empty
        method, names, args, kw = here[-2]
        assert method == "close_gaps"
        refused(c, "scaffolds", method, swapped(args, 3, there[-2][2][3][:0]), kw)


def same_results(want, got, what):
    want, got = (list(x.values()) if isinstance(x, dict) else list(x) for x in (want, got))
    assert len(want) == len(got), what
    for w, g in zip(want, got):
        if isinstance(w, dict) or w is None:
            assert w == g, what
        else:
            assert type(w) is type(g) and w.dtype == g.dtype and w.shape == g.shape and raw(w) == raw(g), what


def test_an_empty_input_on_the_other_side_is_accepted(chain):
    c = chain
    for host in (True, False):
        # no records on the other side: the call is the one with no records on this side
        calls = {m: (names, args, kw) for m, names, args, kw in calls_of(c, host)}
        others = {m: args for m, _, args, _ in calls_of(c, not host)}
        for method, name in (("align_gapped", "alns"), ("pair_inserts", "gap_alns"), ("local_assm", "gap_alns"), ("ctg_links", "gap_alns"),
                             ("close_gaps", "gap_alns"), ("shuffle_reads", "gap_alns")):
            names, args, kw = calls[method]
            i = names.index(name)
            if method in ("local_assm", "shuffle_reads", "ctg_links"):  # their pairs point at records: those of no records
                j = names.index("pairs")
                args = swapped(args, j, c.kc.pair_inserts(args[names.index("offsets")], args[i][:0], max_insert=MAX_INSERT)[1])
            want = getattr(c.kc, method)(*swapped(args, i, args[i][:0]), **kw)
            same_results(want, getattr(c.kc, method)(*swapped(args, i, others[method][i][:0]), **kw), (method, name))
        # no reads: the bases, the quals, the pairs and the records of none may come from either side
        calls = {m: (names, args, kw) for m, names, args, kw in zero_read_calls(c, host)}
        others = {m: args for m, _, args, _ in zero_read_calls(c, not host)}
        for method, free in (("align_reads", ("bases",)), ("align_gapped", ("bases", "alns")), ("pair_inserts", ("gap_alns",)),
                             ("local_assm", ("bases", "quals", "gap_alns", "pairs")), ("ctg_links", ("gap_alns", "pairs")),
                             ("close_gaps", ("gap_alns",)), ("shuffle_reads", ("bases", "quals", "gap_alns", "pairs"))):
            names, args, kw = calls[method]
            want = getattr(c.kc, method)(*args, **kw)
            for name in free:
                i = names.index(name)
                same_results(want, getattr(c.kc, method)(*swapped(args, i, others[method][i]), **kw), (method, name))


def test_kernel_times_returns_every_entry_the_library_has(chain):
    n = C.c_int(0)
    _lib.check(pkg.lib().kc_get_kernel_times(chain.kc._h, None, 0, C.byref(n)), "kc_get_kernel_times")
    times = chain.kc.kernel_times()
    assert n.value > 0 and len(times) == n.value
    assert all(type(v[0]) is int and v[0] > 0 and type(v[1]) is float for v in times.values())
