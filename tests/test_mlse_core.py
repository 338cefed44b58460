"""The one trellis of the sequence equalisers' float32 models (tests/mlse_core.py's half) against an independent statement of what
it computes: on a short chain every allowed bit sequence is walked in plain Python, and M_0 - M_1 from the per-sequence sums equals
half's D EXACTLY.

Why exactly.  float32 addition is monotone: a <= b gives fl(a + c) <= fl(b + c).  So fl(min(a, b) + c) = min(fl(a + c), fl(b + c)),
and by induction the forward metric of a state is the minimum, over the sequences that reach it, of the branch metrics summed left
to right from 0; the backward metric the minimum over the continuations of those summed right to left onto 0; their sum the
minimum over the pairs.  The minima per bit value of these per-sequence numbers are what the recursion holds -- word for word, ties
and infinities included.  No GPU."""
import itertools

import numpy as np
import pytest

import mlse_core as core
import mlse_model

F = np.float32
INF = F(np.inf)


def branch(y, g, n, x):
    """|y[n] - Z[x]|^2 in the header's float32 order: Z from +-g[0], then k = 1..4; re first."""
    sign = [F(1.0) if (x >> k) & 1 else F(-1.0) for k in range(5)]
    zr, zi = F(g[0].real * sign[0]), F(g[0].imag * sign[0])
    for k in range(1, 5):
        zr = F(zr + F(g[k].real * sign[k])); zi = F(zi + F(g[k].imag * sign[k]))
    dr, di = F(y[n].real - zr), F(y[n].imag - zi)
    return F(F(dr * dr) + F(di * di))


def by_enumeration(y, g, w, start, steps, first, left, force_tail):
    """D [steps] of one burst from every allowed bit sequence: per sequence and step, the left-to-right sum of the branch metrics up
    to the step plus the right-to-left sum of those after it; the minimum per bit value; M_0 - M_1."""
    M = np.full((steps, 2), INF, F)
    tail = range(steps - 3, steps) if force_tail else ()
    for bits in itertools.product((0, 1), repeat=steps):
        if any(bits[i] for i in tail):
            continue                                           # the tail symbols are -1
        state, gs = int(start), []
        for i, b in enumerate(bits):
            x = (state << 1) | b                               # the step's symbol in bit 0, the four before it above
            gs.append(branch(y, g, (first - i + 4 + w) if left else (first + i + w), x))
            state = x & 15
        for i in range(steps):
            fwd = F(0.0)
            for j in range(i + 1):
                fwd = F(fwd + gs[j])
            bwd = F(0.0)
            for j in range(steps - 1, i, -1):
                bwd = F(gs[j] + bwd)
            M[i, bits[i]] = min(M[i, bits[i]], F(fwd + bwd))
    with np.errstate(all="ignore"):
        return (M[:, 0] - M[:, 1]).astype(F)


@pytest.mark.parametrize("steps,force_tail", [(6, True), (6, False), (4, True), (4, False)])
def test_half_is_the_minimum_over_sequences(steps, force_tail):
    """Random finite float32 samples and taps, one antenna (tests/mlse_model.py's metric), five bursts with their own windows and
    start states, both directions: D is byte-equal to the enumeration's (with the tail forced its last three steps are -inf)."""
    rng = np.random.default_rng(100 * steps + force_tail)
    B = 5
    y = (rng.standard_normal((B, 148)) + 1j * rng.standard_normal((B, 148))).astype(np.complex64)
    g = (rng.standard_normal((B, 5)) + 1j * rng.standard_normal((B, 5))).astype(np.complex64)
    w = np.array([0, -1, -2, -3, -4], np.int32)
    start = np.array([0, 15, 5, 10, int(rng.integers(0, 16))])
    for left, first in ((False, 87), (True, 60), (False, 4), (True, 3 + steps)):
        with np.errstate(all="ignore"):
            D = core.half(mlse_model.metric(y.real.copy(), y.imag.copy(), g.real.copy(), g.imag.copy()), w, start, steps, first, left,
                          force_tail)
        assert D.shape == (B, steps) and D.dtype == F
        for b in range(B):
            want = by_enumeration(y[b], g[b], int(w[b]), start[b], steps, first, left, force_tail)
            assert D[b].tobytes() == want.tobytes(), (left, first, b, D[b], want)
        assert np.all(np.isneginf(D[:, steps - 3:])) == force_tail and np.isfinite(D[:, :steps - 3]).all()
    same = core.half(mlse_model.metric(y.real.copy(), y.imag.copy(), g.real.copy(), g.imag.copy()), w, 5, steps, 87, False, force_tail)
    one = core.half(mlse_model.metric(y.real.copy(), y.imag.copy(), g.real.copy(), g.imag.copy()), w, np.full(B, 5), steps, 87, False, force_tail)
    assert same.tobytes() == one.tobytes()                     # a start word stands for all bursts
