"""tests/chan_ref.py (the float64 channeliser reference the shared-filter form is graded against) pinned on the reference's
own primitives: given the float32 carrier frequencies it must agree with the oracle chain the per-carrier test builds
(Oracle.mix_down from raw sample 192 x CW, then polyphase_resample per window, pullBuffer's slicing) -- the chain the
per-carrier kernel equals bit for bit.  That shows the windows, the history, the output indexing and the phase origin are
the reference's own.  CPU only."""
import numpy as np
import pytest

import chan_ref
import oraclebind
import synth

U = chan_ref.U
TABLE = 1024                                         # the reference's trig table (sigProcLib.cpp: TABLESIZE)


def oracle_chain(o, iq, sps, cw, lpf, freq, swap_iq):
    P, Q, chunk, hist, skip, _ = chan_ref.geometry(sps, cw)
    re, im = (iq[:, 1], iq[:, 0]) if swap_iq else (iq[:, 0], iq[:, 1])
    xc = (re.astype(np.float32) + 1j * im.astype(np.float32)).astype(np.complex64)
    z = o.mix_down(xc, hist, freq)
    h = np.zeros(hist, np.complex64)
    out = []
    for c in range(xc.size // chunk):
        win = np.concatenate([h, z[c * chunk:(c + 1) * chunk]])
        out.append(o.polyphase_resample(win, P, Q, lpf)[skip:])
        h = win[-hist:]
    return np.concatenate(out)


def full_scale(rng, n):
    iq = rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16)
    iq[rng.integers(0, n, size=max(1, n // 50)), rng.integers(0, 2, size=max(1, n // 50))] = -32768
    return iq


@pytest.mark.parametrize("sps,cw,taps,bins,swap", [
    (4, 8, "32", (1, -3, 8), True),
    (4, 1, "odd", (0, 5), False),
    (4, 10, "short", (-8, 2), True),
    (2, 5, "32", (7, -6), True),
    (2, 3, "odd", (4,), False),
    (1, 2, "short", (-1, 3), True),
    (1, 1, "32", (6, -7), False),
])
def test_reference_equals_the_oracle_chain(sps, cw, taps, bins, swap):
    """Two comparisons per output o, both against the oracle chain's float32 result y32:
    (a) the reference fed the oracle's own mixer values (mix_down of a unit stream, exact in float32) must be within
        (kt + 4) u A(o): kt float adds of the polyphase sum, the complex product x * e (at most 2 sqrt 2 u |x| <= 3 u), the
        real product h * z (u) -- that isolates the windows, history, indexing and slicing;
    (b) the reference with its own float64 exp(j theta n), theta the float32 frequency widened, must be within
        (kt + 4 + c_mix) u A(o), c_mix u bounding |expjLookup(phase) - exp(j theta n)|: linear interpolation of a
        1024-entry table, 1 - cos(pi / 1024) = (2 pi / 1024)^2 / 8 = 4.71e-6 (79 u); the phase (float)(t mod 2 pi) and its
        scaling by (float) 1 / 2 pi, <= 6 pi u (19 u); the table entries and the interpolation's three roundings, <= 8 u:
        c_mix = 106.  A wrong phase origin (one sample off: |1 - exp(j theta)| >= 0.38 for the bins used) or a wrong
        window / tap is far outside either bound."""
    rng = np.random.default_rng(sps * 100 + cw)
    P, Q, chunk, hist, skip, _ = chan_ref.geometry(sps, cw)
    L = {"32": 32 * P, "odd": 20 * P + 37, "short": 3 * P + 5}[taps]
    lpf = synth.design_lpf(L, P, beta=6.0, cutoff=0.09 * 8 / cw)
    kt = (L + P - 1) // P
    iq = full_scale(rng, 3 * chunk)
    o = oraclebind.Oracle(sps)
    freqs = np.float32([2.0 * np.pi * b / 16.0 for b in bins])
    y32 = np.stack([oracle_chain(o, iq, sps, cw, lpf, f, swap) for f in freqs]).astype(np.complex128)
    n_raw = hist + iq.shape[0]
    table = np.stack([o.mix_down(np.ones(n_raw, np.complex64), 0, f) for f in freqs])
    ya, A = chan_ref.channelise(iq, sps, cw, lpf, chan_ref.table_mixer(table), swap_iq=swap)
    yb, A2 = chan_ref.channelise(iq, sps, cw, lpf, chan_ref.theta_mixer(freqs.astype(np.float64)), swap_iq=swap)
    assert np.array_equal(A, A2) and y32.shape == ya.shape
    assert (A > 0).mean() > 0.99
    c_mix = (2.0 * np.pi / TABLE) ** 2 / 8.0 / U + 19 + 8
    assert c_mix < 106
    # the mixer bound itself, on every raw sample the windows use
    n = np.arange(n_raw)
    mix_err = max(float(np.abs(table[c].astype(np.complex128) - np.exp(1j * float(f) * n)).max()) for c, f in enumerate(freqs))
    assert mix_err <= 106 * U, mix_err / U
    Am = np.maximum(A, 1e-300)
    ra = float((np.abs(ya - y32) / Am).max()) / U
    rb = float((np.abs(yb - y32) / Am).max()) / U
    print("reference vs oracle chain (sps %d, CW %d, L %d): (a) oracle mixer %.2f u A (bound %d), (b) float64 mixer %.2f u A "
          "(bound %d); mixer alone %.1f u" % (sps, cw, L, ra, kt + 4, rb, kt + 4 + 106, mix_err / U))
    assert ra <= kt + 4
    assert rb <= kt + 4 + 106
    # and a reference that is wrong by one sample of phase, or by one output, is far outside (b)'s bound
    yc, _ = chan_ref.channelise(iq, sps, cw, lpf, chan_ref.theta_mixer((freqs.astype(np.float64))), swap_iq=not swap)
    assert float((np.abs(yc - y32) / Am).max()) / U > 1e4


def test_reference_zero_stream_and_grid_mixer():
    """An all-zero stream gives exact zeros and A = 0; the grid mixer equals exp(j theta n) with the exact grid theta."""
    P, Q, chunk, hist, skip, n_out = chan_ref.geometry(2, 3)
    lpf = synth.design_lpf(20 * P + 37, P, beta=6.0, cutoff=0.2)
    y, A = chan_ref.channelise(np.zeros((2 * chunk, 2), np.int16), 2, 3, lpf, chan_ref.grid_mixer([0, 8, -3]))
    assert y.shape == (3, 2 * (n_out - skip)) and not y.any() and not A.any()
    n = np.arange(5000)
    mix, _ = chan_ref.grid_mixer([-8, 8, 5, -3])
    for c, b in enumerate((-8, 8, 5, -3)):
        assert np.abs(mix(c, n) - np.exp(2j * np.pi * b / 16.0 * n)).max() < 1e-11
