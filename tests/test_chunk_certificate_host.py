"""The mirror lattices of tests/test_gpu_chunk.py checked on the host, with the planner's own unit layout and a plain fp64 model
of the recursion (tests/chunk_lattice.py): every cut's spread stays inside the time-split certificate's tolerance, yet the
spreads add up across the cuts until the last unit sees the wrong group ahead by more than two of the stitch's margins.
If the planner or the builder changes, this fails here instead of the GPU test quietly going easy."""
import numpy as np
import pytest

import chunk_lattice as L
from oracle import factored as F

# (frames, classes per group, span limit, drifting group): the ring kernels (K = 130, ~52 cuts) and BAND mode (K = 1024, ~57
# cuts); group B drifting: the spreads on the other side of the cuts' reference state
MIRROR_SHAPES = [(14000, 5, 130, 0), (60000, 5, 1024, 0), (14000, 5, 130, 1)]


@pytest.mark.parametrize('shape', MIRROR_SHAPES)
def test_mirror_lattice_accumulates_an_offset_the_certificate_lets_through(shape):
    t, c, k, drifting = shape
    units = L.unit_layout([t], 2 * c, k)[0]
    assert len(units) >= 50, len(units)
    p = L.mirror_problem(5, t, c, k, units, drifting=drifting)
    rep = L.certificate_report(p, units)
    # every cut certifies: its spread is at most half the smallest tolerance the kernel can take there
    assert (rep['spreads'] < 0.5 * rep['tols']).all(), rep['spreads'] / rep['tols']
    assert (rep['spreads'] > 0.4 * rep['tols']).all(), rep['spreads'] / rep['tols']
    # the one-piece decode ends in the other group; the last unit sees the drifting group ahead, clear of twice the stitch's margin
    assert rep['margin_whole'] < 0
    assert rep['margin_unit'] > 2 * rep['tau_unit'], (rep['margin_unit'], rep['tau_unit'])
    # ... by the sum of the spreads, which is what the cuts let through
    assert rep['margin_unit'] - rep['margin_whole'] == pytest.approx(rep['spreads'].sum(), rel=1e-3)
    # the twin decodes the designed label sequence, never changes group and ends in the other group
    spans, _ = F.viterbi(p['elp'], p['lengths'], p['trans'], p['init'], p['lens'])
    labs = spans[0, :t][spans[0, :t] >= 0]
    other = (1 - drifting) * c
    assert ((labs >= other) & (labs < other + c)).all()
    np.testing.assert_array_equal(labs - other, [q for q, _ in p['segs']])
    assert spans[0, t] == 2 * c


def test_three_span_run_lattice_straddles_a_cut():
    """tests/test_gpu_chunk.py's one-class run decoded as three spans: the twin cuts the run, which starts inside the certified
    window in front of a cut and crosses it, into three spans of one class, and decodes every other segment as designed."""
    t, c, k = 6000, 5, 130
    units = L.unit_layout([t], c, k)[0]
    p, s0, e0 = L.three_span_problem(3, t, c, k, units)
    spans, _ = F.viterbi(p['elp'], p['lengths'], p['trans'], p['init'], p['lens'])
    st = np.nonzero(spans[0, :t] >= 0)[0]
    inside = st[(st >= s0) & (st < e0)]
    assert len(inside) == 3 and inside[0] == s0 and e0 in st
    assert sorted(np.diff(np.append(inside, e0))) == [60, 60, 61]
    run_cls = p['labels'][s0]
    assert (spans[0, inside] == run_cls).all()
    j = len(units) // 2
    r = units[j][0] + units[j][2]
    assert r - (min(k, t) - 1) <= s0 <= r < e0
    # every other segment as designed: the run's one segment becomes three
    want = []
    for q, ln in p['segs']:
        want += [q] * (3 if q == run_cls else 1)
    np.testing.assert_array_equal(spans[0, st], want)
