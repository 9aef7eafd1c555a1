"""The inputs of the device sort's tests do what those tests assume: for every family of tests/sort_cases.py the
oracle's results are exactly the intended canonical k-mers with the intended counts and extensions."""
import numpy as np
import pytest

import sort_cases as S
from count_cases import revcomp
from oracle import cpu_oracle as O


@pytest.mark.parametrize("k", S.KS)
def test_families_leave_exactly_the_intended_results(k):
    fams = S.families(k)
    names = [f.name for f in fams]
    assert names[:5] == ["empty", "one k-mer", "two k-mers, the larger first", "low bits", "high bits"] and names[-1] == "counts"
    assert ("word 1 only" in names) == (k >= 33) and ("bases 31 and 32" in names) == (k >= 32)
    for f in fams:
        res, _ = O.count_reads(f.reads(), None, k=k)
        want = f.expected()
        assert res[0].shape == want[0].shape, f.name
        for g, w in zip(res, want):
            assert (g == w).all(), f.name
        assert len(want[1]) == len(f.entries)


@pytest.mark.parametrize("k", S.KS)
def test_families_vary_the_bits_they_are_named_for(k):
    """low bits: keys equal outside the last four bases; high bits: outside the first four; word 1 only: word 0 equal;
    the boundary pairs: one base apart at 31 or 32; counts: one k-mer for each number of digits, and the clip."""
    by = {f.name: f for f in S.families(k)}
    low = [e[0] for e in by["low bits"].entries]
    assert len(low) == 256 and len({x[:-4] for x in low}) == 1
    high = [e[0] for e in by["high bits"].entries]
    assert len(high) == 256 and len({x[4:] for x in high}) == 1
    two = by["two k-mers, the larger first"].entries
    assert two[0][0] > two[1][0]
    assert all(len(r) < k + 2 for r in by["empty"].reads()) and by["empty"].reads()
    if k >= 33:
        w1 = [e[0] for e in by["word 1 only"].entries]
        assert len({x[:32] for x in w1}) == 1 and len(w1) == (4 if k == 33 else 256)
    if k >= 32:
        xs = sorted(e[0] for e in by["bases 31 and 32"].entries)
        at = set()
        for a in xs:
            for b in xs:
                d = [i for i in range(k) if a[i] != b[i]]
                if len(d) == 1:
                    at.add(d[0])
        assert at == ({31} if k == 32 else {31, 32})
    cs = by["counts"]
    assert [e[3] for e in cs.entries] == list(S.COUNTS)
    assert sorted(len(str(int(c))) for c in cs.expected()[1]) == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 5]
    assert int(cs.expected()[1].max()) == 65535
    for f in by.values():
        for x, _, _, _ in f.entries:
            assert x < revcomp(x)
    assert isinstance(by["counts"].arrays()[2], np.ndarray)
