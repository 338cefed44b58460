"""The fading-tap generator's model (tests/air_fade_model.py) against arithmetic that does not share its code.  No GPU.

  trig          the float32 restatement: the phases on the axes exact, every component within the header's 1e-5 of float64
                over the 2^24 phases (every 5th, and every odd one of a block at each octant's edge)
  integers      step = floor(C D / 2^23) in Python integers at D = 0, 1, 2^31 - 1 and C = +-2^23; theta at row 0 and at the
                hyperframe's last row; the column rotation against exact fractions
  weights       a whole-sample delay gives one weight of 1.0; a fractional one a windowed sinc that sums to about 1
  split         a call of F frames equals any split of it, across the hyperframe's wrap too
  statistics    4,096 links, one path: the mean tap power equals the path power and the autocorrelation over lags of slots
                equals J0(2 pi f_d dt), each inside 5 standard errors estimated from the sample; two equal paths 2,500 ns apart:
                the tap of one link on columns 200, 400 and 77 kHz away correlates with column 0 as the rotation phases predict"""
from fractions import Fraction

import numpy as np
import pytest
from scipy.special import j0

import air_fade_model as fm
import air_model as am


def test_trig_restatement():
    c, s = fm.cossin24([0, 1 << 22, 2 << 22, 3 << 22])
    assert np.array_equal(c, np.array([1, 0, -1, 0], np.float32)) and np.array_equal(s, np.array([0, 1, 0, -1], np.float32))
    assert c.dtype == np.float32
    worst = 0.0
    edges = np.concatenate([o * (1 << 21) + np.arange(-4096, 4096) for o in range(9)]) & 0xffffff
    for k in (np.arange(0, 1 << 24, 5), edges):
        c, s = fm.cossin24(k)
        x = 2.0 * np.pi * k.astype(np.float64) * 2.0 ** -24
        worst = max(worst, np.abs(c - np.cos(x)).max(), np.abs(s - np.sin(x)).max())
    print("worst |float32 steps - float64| over the phases: %.3e (the header promises 1e-5)" % worst)
    assert worst <= fm.D_TRIG


def test_integer_rules_at_their_edges():
    Q = 1 << 23
    m = fm.FadeModel(1, [0, 0, 0], [1.0, 1.0, 1.0], 4, 1, los_share=[0.5, 0.5, 0.5], los_cos_q23=[Q, -Q, 12345])
    L, seed = 5, 0x1234567890abcdef
    phi, C = m.cosines(seed, L)
    assert (np.abs(C) <= Q).all() and (C[:, 0, 4] == Q).all() and (C[:, 1, 4] == -Q).all()
    dop = np.array([0, 1, (1 << 31) - 1, 0x80000000 | 77, 3000000], np.uint32)
    phi2, step = m.params(seed, L, dop)
    assert np.array_equal(phi, phi2)
    for l in range(L):
        D = int(dop[l]) & 0x7fffffff
        want = [[(int(C[l, p, s]) * D) // Q for s in range(5)] for p in range(3)]           # floor, in Python integers
        assert step[l].tolist() == want
    assert not step[0].any()                                                               # D = 0: nothing moves
    assert (step[2, 0, 4] == (1 << 31) - 1) and (step[2, 1, 4] == -((1 << 31) - 1))         # C = +-2^23: +-D
    assert step[3, 0, 4] == 77                                                             # the top bit of D is not read
    # the phase at row 0 and at the last row, in Python integers
    for row in (0, fm.ROWS - 1):
        th = fm.FadeModel.theta(phi, step, [row])
        for l, p, s in [(2, 0, 4), (2, 1, 4), (4, 2, 0), (1, 0, 1)]:
            assert int(th[l, 0, p, s]) == (int(phi[l, p, s]) + row * int(step[l, p, s])) % (1 << 32)
    assert np.array_equal(fm.FadeModel.theta(phi, step, [0])[:, 0], phi.astype(np.int64))
    # D = 0: the taps do not move from slot to slot
    h = m.taps(fm.ROWS // 8 - 1, 1, 1, seed, 1, dop[:1], link=[[0] * 8])
    assert (h[0] == h[0, 0]).all() and abs(h[0, 0, 0]) > 0


def test_column_rotation_is_exact():
    for khz, ns in [(0, 5000), (200, 0), (200, 5000), (200, 2500), (-200, 2500), (1800000, 17200), (-9999999, 999999), (3, 1), (600, 1)]:
        turn = Fraction(-khz * ns, 10 ** 6) % 1
        x = turn * 2 ** 32
        want = (x.numerator * 2 + x.denominator) // (2 * x.denominator) % 2 ** 32              # floor(x + 1/2)
        assert fm.rot_phase(khz, ns) == want, (khz, ns)
    assert fm.rot_phase(200, 5000) == 0 and fm.rot_phase(200, 2500) == 1 << 31 and fm.rot_phase(-200, 1250) == 1 << 30


def test_weights():
    for sps, ns, centre, at in [(1, 0, 0, 0), (4, 0, 4, 4), (4, 12000, 4, 17), (1, 48000, 2, 15), (4, 24000, 0, 26)]:
        w = fm.weights([ns], sps, 32, centre)
        assert w.dtype == np.float32 and np.count_nonzero(w) == 1 and w[0, at] == np.float32(1.0), (sps, ns, centre)
    w = fm.weights([1600], 4, 32, 4)[0]                          # 1.7333 samples after tap 4
    assert np.count_nonzero(w) == 8 and w[:2].tolist() == [0, 0] and np.argmax(w) == 6 and abs(w.sum() - 1.0) < 0.05
    assert np.count_nonzero(fm.weights([1600], 4, 32, 0)[0]) == 6                         # centre 0: the precursors are cut


def test_split_equals_whole():
    pr = fm.profile("TU6")
    m = fm.FadeModel(4, n_sinusoids=8, n_taps=12, centre=2, **pr)
    seed, L = 77, 24
    dop = (np.arange(L, dtype=np.uint32) * 7919 * 4099) % (1 << 31)
    fn = am.HYPER - 2
    whole = m.taps(fn, 3, 4, seed, L, dop)
    parts = [m.taps(fn, 3, 1, seed, L, dop), m.taps(fn + 1, 3, 1, seed, L, dop), m.taps(0, 3, 2, seed, L, dop)]
    assert np.array_equal(whole, np.concatenate(parts, axis=1))
    assert not np.array_equal(whole[:, :8], whole[:, 8:16])


def _se(x):
    return x.std(ddof=1) / np.sqrt(len(x))


def test_statistics_of_the_process():
    L, S, seed, power = 4096, 16, 20261019, 0.6
    fd = 0.023                                                  # turn per slot: 40 Hz of Doppler at 577 us a slot
    D = int(round(fd * 2 ** 32))
    m = fm.FadeModel(1, [0], [power], S, 1)
    phi, step = m.params(seed, L, np.full(L, D, np.uint32))
    lags = np.array([0, 1, 3, 8, 13, 17, 24, 40, 64])
    g = m.gains(phi, step, 1000 + lags, 0)[:, :, 0]             # [L][lags]
    pw = np.abs(g[:, 0]) ** 2
    print("mean power %.4f (path power %.4f, standard error %.4f)" % (pw.mean(), np.float32(power), _se(pw)))
    assert abs(pw.mean() - float(np.float32(power))) <= 5 * _se(pw)
    for k, lag in enumerate(lags[1:], 1):
        z = g[:, 0] * np.conj(g[:, k]) / float(np.float32(power))
        want = j0(2 * np.pi * (D * 2.0 ** -32) * lag)
        print("lag %3d slots: autocorrelation %+.4f %+.4fj, J0 %+.4f, standard error %.4f" % (lag, z.real.mean(), z.imag.mean(), want, _se(z.real)))
        assert abs(z.real.mean() - want) <= 5 * _se(z.real) and abs(z.imag.mean()) <= 5 * _se(z.imag)
    # frequency selectivity: two equal paths 2,500 ns apart, both on tap 0 at sps 1 (weights 1 and w1)
    m2 = fm.FadeModel(1, [0, 2500], [0.5, 0.5], S, 1, col_khz=[0, 200, 400, 77])
    phi, step = m2.params(seed, L, np.full(L, D, np.uint32))
    h = [(m2.gains(phi, step, [5], a)[:, 0, :] * m2.w[:, 0].astype(np.float64)).sum(axis=1) for a in range(4)]
    for a in (1, 2, 3):
        z = h[0] * np.conj(h[a])
        d = [(fm.rot_phase(0, ns) >> 8) - (fm.rot_phase(m2.col_khz[a], ns) >> 8) for ns in (0, 2500)]
        want = sum(0.5 * float(m2.w[p, 0]) ** 2 * np.exp(2j * np.pi * d[p] * 2.0 ** -24) for p in range(2))
        print("column %d (%d kHz): correlation with column 0 %+.4f %+.4fj, predicted %+.4f %+.4fj" % (a, m2.col_khz[a], z.real.mean(), z.imag.mean(), want.real, want.imag))
        assert abs(z.real.mean() - want.real) <= 5 * _se(z.real) and abs(z.imag.mean() - want.imag) <= 5 * _se(z.imag)


def test_profiles_are_data():
    for name in fm.PROFILES:
        pr = fm.profile(name)
        assert len(pr["delay_ns"]) == 6 and abs(float(pr["power"].sum()) - 1.0) < 1e-6 and "from memory" in fm.__doc__
