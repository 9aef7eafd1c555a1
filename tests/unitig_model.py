"""Host model of kc_build_unitigs: DESIGN section 14's definition, statement by statement, as a walk over a Python dict.

This project's own definition (the reference holds no traversal code: the stage is commented out in its proxy).  Nothing
here is shared with the kernels: k-mers are Python strings, results a dict {canonical k-mer: (count, left, right)}, an
oriented node a tuple (x, s) with s = +1 or -1."""
import numpy as np

_COMP = str.maketrans("ACGT", "TGCA")


def comp(c):
    return c.translate(_COMP)


def revcomp(s):
    return s[::-1].translate(_COMP)


def canonical(s):
    r = revcomp(s)
    return r if r < s else s


# ---- oriented nodes -----------------------------------------------------------------------------------------------
def seq(v):
    x, s = v
    return x if s > 0 else revcomp(x)


def ext_r(R, v):
    x, s = v
    return R[x][2] if s > 0 else comp(R[x][1])


def ext_l(R, v):
    x, s = v
    return R[x][1] if s > 0 else comp(R[x][2])


def twin(v):
    return (v[0], -v[1])


# ---- links --------------------------------------------------------------------------------------------------------
def successor(R, v):
    """the node v links to, or None"""
    x = v[0]
    e = ext_r(R, v)
    if e not in "ACGT":  # no base: w_seq is no k-mer, so y is not in R
        return None
    w_seq = seq(v)[1:] + e
    y = canonical(w_seq)
    t = 1 if w_seq == y else -1
    if y not in R:
        return None
    if ext_l(R, (y, t)) != seq(v)[0]:
        return None
    if y == x:
        return None
    if x == revcomp(x) or y == revcomp(y):
        return None
    return (y, t)


def predecessor(R, v):
    w = successor(R, twin(v))
    return None if w is None else twin(w)


# ---- components ---------------------------------------------------------------------------------------------------
def component(R, v):
    """(nodes in link order, is_cycle) of the component v lies on; a cycle starts at (x*, +) or, for the twin of that
    cycle, behind (x*, -) -- the cut of the definition"""
    back = [v]
    seen = {v}
    while True:
        p = predecessor(R, back[-1])
        if p is None or p in seen:
            break
        back.append(p)
        seen.add(p)
    cyc = p is not None
    nodes = back[::-1]
    if not cyc:
        while True:
            nx = successor(R, nodes[-1])
            if nx is None:
                break
            assert nx not in seen, "a path that meets itself"
            nodes.append(nx)
            seen.add(nx)
        return nodes, False
    assert p == v, "a cycle closes where the walk began (every node has one predecessor)"
    xs = min(x for x, _ in nodes)
    plus = [i for i, w in enumerate(nodes) if w == (xs, 1)]
    if plus:  # cut in front of (x*, +)
        i = plus[0]
    else:  # the twin cycle: its cut lies behind (x*, -)
        i = (nodes.index((xs, -1)) + 1) % len(nodes)
    return nodes[i:] + nodes[:i], True


def unitigs(results, k):
    """results: {canonical k-mer string: (count, left, right)} with left/right one-character strings.
    Returns (list of (sequence, kmer_sum, depth, m), stats dict), in the output's order."""
    R = results
    for x in R:
        assert len(x) == k and x == canonical(x)
    done = set()
    out = []
    circular = 0
    for x in sorted(R):  # ascending canonical key: the order of kc_sort_results (A < C < G < T, as the 2-bit codes)
        if x in done:
            continue
        nodes, cyc = component(R, (x, 1))
        tw = [twin(w) for w in reversed(nodes)]
        if len(nodes) > 1 and tw[0][0] < nodes[0][0]:  # of a path and its twin, the one with the smaller head k-mer
            nodes = tw
        elif len(nodes) == 1:
            nodes = [(x, 1)]
        for w in nodes:
            assert w[0] not in done, "a k-mer on two unitigs"
            done.add(w[0])
        circular += 1 if cyc else 0
        text = seq(nodes[0]) + "".join(seq(w)[-1] for w in nodes[1:])
        m = len(nodes)
        ksum = sum(R[w[0]][0] for w in nodes)
        depth = min(65535, (2 * ksum + m) // (2 * m))
        out.append((nodes[0][0], text, ksum, depth, m))
    out.sort(key=lambda u: u[0])
    units = [(t, s, d, m) for _, t, s, d, m in out]
    stats = dict(kmers=len(R), unitigs=len(units), singletons=sum(1 for u in units if u[3] == 1), circular=circular,
                 bases=sum(len(u[0]) for u in units), longest=max([len(u[0]) for u in units], default=0))
    return units, stats


def block(units):
    """the device output of kc_build_unitigs for these unitigs: (seqs bytes, depths u16, offsets u64, kmer_sums u64)"""
    seqs = "".join(u[0] + "_" for u in units).encode()
    depths = np.zeros(len(seqs), dtype=np.uint16)
    offsets = np.zeros(len(units) + 1, dtype=np.uint64)
    at = 0
    for i, (t, _, d, _) in enumerate(units):
        offsets[i] = at
        depths[at:at + len(t)] = d
        at += len(t) + 1
    offsets[len(units)] = at
    return seqs, depths, offsets, np.array([u[1] for u in units], dtype=np.uint64)


def results_dict(keys, counts, left, right, k):
    """numpy results (as KmerCounter.results() gives them) -> the model's dict"""
    n = len(counts)
    keys = np.asarray(keys, dtype=np.uint64).reshape(n, -1)
    mat = np.empty((n, k), dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(k):
        mat[:, j] = acgt[((keys[:, j // 32] >> np.uint64(2 * (31 - j % 32))) & np.uint64(3)).astype(np.int64)]
    text = mat.tobytes().decode()
    cs, ls, rs = np.asarray(counts).tolist(), np.asarray(left).tolist(), np.asarray(right).tolist()
    return {text[i * k:(i + 1) * k]: (cs[i], chr(ls[i]), chr(rs[i])) for i in range(n)}
