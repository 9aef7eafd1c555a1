"""A genome with one planted repeat, cut into contigs of drawn lengths, orientations and gaps, under noisy read pairs of
drawn fragment lengths: the construction behind tests/test_chain_model.py (the host models as a chain) and
tests/test_gpu_chain_noisy.py (the device's own chain, every step against its model).  Everything follows from the seed.

Unlike tests/links_cases.py's construction this one puts between the stages what real data puts there: clipped records
of kind DP, reads with several records, repeated seeds, pairs of several classes, chimeric pairs, overlaps the text
confirms and overlaps it does not, splint reads that disagree on a column, and scaffolds of several members in both
orientations.  The claims below are decided from the layout alone, never from a result."""
import numpy as np

from links_cases import K, READ_LEN, genome, revc

FRAGMENT = 400      # the mean fragment length: the insert_avg of the calls
MAX_INSERT = 1000   # of the calls; a chimeric pair's mates lie further apart
REPEAT_LEN = 300
Q_HI, Q_MID, Q_LOW = 40, 15, 5  # above hi_qual, between min_qual and hi_qual, below min_qual (kc_local_assm's classes)
# the parameters of the chain's calls, shared by the model chain and the device's
LINK_KW = dict(insert_avg=FRAGMENT, max_insert=MAX_INSERT, end_slack=5, max_overlap=50, max_splint_gap=50)
CLOSE_KW = dict(end_slack=5, max_overlap=50, max_splint_gap=50)


class Case:
    """G, repeat ((start, stop) of both copies), layout [(start, stop, reversed)], gaps [gap behind contig i], contigs,
    reads, quals, truth [(start, stop, reversed, (substitutions, indel bases)) or None for a random read]"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def ctg_lens(self):
        return [len(c) for c in self.contigs]

    @property
    def read_lens(self):
        return [len(r) for r in self.reads]

    def subset(self, pairs):
        """the same case with its first `pairs` pairs only"""
        n = 2 * pairs
        return Case(**dict(self.__dict__, reads=self.reads[:n], quals=self.quals[:n], truth=self.truth[:n]))


def draw_layout(rng, n):
    """contigs of 300..1500 bases with gaps of -30..+40 along [0, n), redrawn until one join abuts (gap 0) and one
    overlaps by more than K"""
    while True:
        layout, gaps, at = [], [], 0
        while True:
            ln = int(rng.integers(300, 1501))
            if n - (at + ln) < 340:  # what is left is no contig and a gap: this one runs to the end
                ln = n - at
            layout.append((at, at + ln, int(rng.integers(0, 2))))
            if at + ln == n:
                break
            gaps.append(int(rng.choice([0, 0, -25, -28]) if rng.integers(0, 4) == 0 else rng.integers(-30, 41)))
            at += ln + gaps[-1]
        if layout[-1][1] - layout[-1][0] > 1500:
            continue
        if 0 in gaps and any(g < -K for g in gaps) and any(r for _, _, r in layout) and not all(r for _, _, r in layout):
            return layout, gaps


def noisy_read(rng, G, start, reversed_, sub_rate, p_del, p_ins, p_n, p_lower, p_tail):
    """(text, quals, truth) of one read of READ_LEN bases that begins at (or, reversed, covers from) genome position start"""
    kind = rng.random()
    span = READ_LEN + (1 if kind < p_del else -1 if kind < p_del + p_ins else 0)
    s = list(G[start:start + span])
    q = [Q_HI] * span
    subs = 0
    for i in np.nonzero(rng.random(span) < sub_rate)[0]:
        s[i] = "ACGT"[("ACGT".index(s[i]) + int(rng.integers(1, 4))) % 4]
        q[i] = [Q_HI, Q_HI, Q_MID, Q_LOW][int(rng.integers(0, 4))]
        subs += 1
    indels = 0
    if span > READ_LEN:
        at = int(rng.integers(1, span - 1))
        del s[at], q[at]
        indels = 1
    elif span < READ_LEN:
        at = int(rng.integers(1, span - 1))
        s.insert(at, "ACGT"[int(rng.integers(0, 4))])
        q.insert(at, Q_HI)
        indels = 1
    if rng.random() < p_n:
        s[int(rng.integers(0, READ_LEN))] = "N"
    text, quals = "".join(s), q
    if reversed_:
        text, quals = revc(text), quals[::-1]
    if rng.random() < p_tail:  # a low-quality tail, at the read's own end
        t = int(rng.integers(5, 31))
        quals[READ_LEN - t:] = [int(x) for x in rng.integers(2, 20, size=t)]
    if rng.random() < p_lower:
        text = text.lower()
    assert len(text) == len(quals) == READ_LEN
    return text, "".join(chr(33 + x) for x in quals), (start, start + span, int(reversed_), (subs, indels))


def noisy_assembly(seed, n=12000, pairs=400, chimeric=6, random_mates=4, frag_sd=30, sub_rate=0.01, p_del=0.03, p_ins=0.02, p_n=0.02,
                   p_lower=0.02, p_tail=0.1):
    """the Case of a seed: `pairs` pairs with fragment lengths from a clipped N(FRAGMENT, frag_sd), then `chimeric` pairs
    whose mates lie more than MAX_INSERT apart, then `random_mates` pairs with one mate from nowhere"""
    rng = np.random.default_rng(seed)
    G = genome(seed, n)
    a = int(rng.integers(200, n - REPEAT_LEN - 200))
    while True:
        b = int(rng.integers(200, n - REPEAT_LEN - 200))
        if abs(a - b) >= 3000 + REPEAT_LEN:
            break
    G = G[:b] + G[a:a + REPEAT_LEN] + G[b + REPEAT_LEN:]
    layout, gaps = draw_layout(rng, n)
    contigs = [revc(G[s:e]) if r else G[s:e] for s, e, r in layout]
    noise = (sub_rate, p_del, p_ins, p_n, p_lower, p_tail)
    reads, quals, truth = [], [], []

    def add(pair):
        if int(rng.integers(0, 2)):  # either read may come first
            pair.reverse()
        for text, q, where in pair:
            reads.append(text)
            quals.append(q)
            truth.append(where)

    for p in range(pairs + chimeric + random_mates):
        f = int(np.clip(round(rng.normal(FRAGMENT, frag_sd)), FRAGMENT - 90, FRAGMENT + 90))
        s0 = int(rng.integers(0, n - f - 1))
        s1 = s0 + f - READ_LEN - 1  # (a read with a deletion covers READ_LEN + 1 bases)
        if pairs <= p < pairs + chimeric:  # the mate from a place further than max_insert away
            while abs(s1 - s0) < MAX_INSERT + 500:
                s1 = int(rng.integers(0, n - READ_LEN - 1))
        first = noisy_read(rng, G, s0, False, *noise)
        if p >= pairs + chimeric:  # a mate from nowhere
            second = ("".join("ACGT"[i] for i in rng.integers(0, 4, size=READ_LEN)), chr(33 + Q_HI) * READ_LEN, None)
        else:
            second = noisy_read(rng, G, s1, True, *noise)
        add([first, second])
    return Case(G=G, repeat=((a, a + REPEAT_LEN), (b, b + REPEAT_LEN)), layout=layout, gaps=gaps, contigs=contigs, reads=reads, quals=quals,
                truth=truth)


# ---- what follows from the construction alone -------------------------------------------------------------------------
def near_repeat(case, lo, hi, margin=0):
    """[lo, hi) of the genome lies inside or within margin bases of a repeat copy"""
    return any(lo < e + margin and s - margin < hi for s, e in case.repeat)


def in_genome(case, text):
    return text in case.G or text in revc(case.G)


def end_position(case, end):
    """the genome position at which contig end `end` (2u: left, 2u + 1: right, in the contig's own orientation) lies"""
    s, e, r = case.layout[end >> 1]
    return e if (end & 1) ^ r else s


def neighbours(case):
    """{(lo end, hi end): gap} of the ends that are neighbours in the layout"""
    out = {}
    for i, gap in enumerate(case.gaps):
        x = 2 * i + (1 ^ case.layout[i][2])          # contig i's end at its genome stop
        y = 2 * (i + 1) + case.layout[i + 1][2]      # contig i + 1's end at its genome start
        out[(min(x, y), max(x, y))] = gap
    return out


def check_gapped(case, gapped, min_placed=0.9):
    """every read off the repeat: its best record lies on a contig it shares K bases with, on the true strand, within its
    indel bases of the true diagonal.  Returns (reads checked, reads skipped for the repeat)."""
    best = {}
    for i, x in enumerate(gapped):
        if int(x["kind"]) != 2 and (int(x["read"]) not in best or int(x["score"]) > int(gapped[best[int(x["read"])]]["score"])):
            best[int(x["read"])] = i
    checked = skipped = 0
    for r, where in enumerate(case.truth):
        if where is None or r not in best:
            continue
        s, e, rr, (_, indels) = where
        if near_repeat(case, s, e):
            skipped += 1
            continue
        x = gapped[best[r]]
        cs, ce, cr = case.layout[int(x["ctg"])]
        assert min(e, ce) - max(s, cs) >= K, (r, where, x)
        assert int(x["orient"]) == rr ^ cr, (r, where, x)
        d = (ce - e) if cr else (s - cs)
        assert abs(int(x["cstart"]) - int(x["rstart"]) - d) <= indels, (r, where, x, d)
        checked += 1
    placed = sum(1 for w in case.truth if w is not None)
    assert checked + skipped >= min_placed * placed, (checked, skipped, placed)
    return checked, skipped


def check_links(case, links):
    """every link with both splints and spans, its ends off the repeat: the ends are neighbours in the layout and the
    splint gaps lie within a read's indel bases (one) of the true gap.  Returns (links checked, links excepted)."""
    want = neighbours(case)
    checked = excepted = 0
    for x in links:
        f, t = int(x["from"]), int(x["to"])
        if f > t or not (int(x["splints"]) and int(x["spans"])):
            continue
        if any(near_repeat(case, end_position(case, v), end_position(case, v), READ_LEN) for v in (f, t)):
            excepted += 1
            continue
        assert (f, t) in want, (x, sorted(want))
        assert want[(f, t)] - 1 <= int(x["splint_gap_min"]) <= int(x["splint_gap_max"]) <= want[(f, t)] + 1, (x, want[(f, t)])
        checked += 1
    print("links with splints and spans: %d checked, %d excepted for the repeat" % (checked, excepted))
    return checked, excepted


def check_local_assm(case, block, offsets, ends):
    """every end further than a read from the repeat: the contig with that end's extension is a piece of the genome.
    Returns the ends checked."""
    text = bytes(bytearray(block)).decode()
    checked = 0
    for u, ctg in enumerate(case.contigs):
        whole = text[int(offsets[u]):int(offsets[u + 1]) - 1]
        left = int(ends[2 * u]["ext_len"])
        assert whole[left:left + len(ctg)] == ctg and len(whole) == left + len(ctg) + int(ends[2 * u + 1]["ext_len"])
        for side, piece in ((0, whole[:left + len(ctg)]), (1, whole[left:])):
            at = end_position(case, 2 * u + side)
            if near_repeat(case, at, at, READ_LEN):
                continue
            assert in_genome(case, piece), (u, side, ends[2 * u + side])
            checked += 1
    return checked


def check_closed(case, strings, stats):
    assert stats["n_bases_left"] == 0, stats
    for s in strings:
        assert in_genome(case, s), (len(s), s[:60])
