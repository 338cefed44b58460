"""The sequence equaliser's float32 model (tests/mlse_model.py) on the CPU: what it is made of (the oracle's demodulator symbols, a
channel estimate that IS the least-squares fit on a clean midamble, the demodulator's soft bits on a one-tap channel, exact
known symbols, the strict-> window rule, the three fallbacks) and what it is for (fewer bit errors than the demodulator on
multipath).  No GPU: the kernel is held to this model word for word in tests/test_gpu_mlse.py."""
import numpy as np
import pytest

import mlse_family
import mlse_model as mm
import oraclebind
import synth

U = 2.0 ** -24                                                # float32 unit roundoff


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_symbols_are_the_demodulators(sps):
    """clamp((y.re + 1) * 0.5) on the model's symbols equals the oracle's demodulateBurst bit for bit: noisy multipath bursts, TOAs
    on and off the 1/512 grid, integer TOAs (no delay filter), 156 and 157 symbols."""
    f = mlse_family.mixed_batch(sps, 3, 24, 5100 + sps)
    o = oraclebind.Oracle(sps)
    for b in range(24):
        x = f["x"][f["off"][b]:f["off"][b] + f["length"][b]]
        for toa in (f["toa"][b], np.float32(np.round(f["toa"][b])), np.float32(0.0)):
            y = mm.symbols(o, x, f["amp"][b], toa)
            want = o.demodulate(x, f["amp"][b], toa)[:148]
            assert mm.slicer(y.real).tobytes() == want.tobytes(), (sps, b, toa)


def clean_symbols(rng, tsc, h, w0, n=6):
    """y[m] = sum_k h[k] a[m - w0 - k] in float64, rounded to complex64 (symbols outside the burst are 0): (bits, y)."""
    bits = synth.normal_bits(rng, n, tsc)
    a = np.zeros((n, 148 + 16)); a[:, 8:156] = 2.0 * bits - 1.0
    y = np.zeros((n, 148), np.complex128)
    for k, hk in enumerate(h):
        y += hk * a[:, 8 - w0 - k:8 - w0 - k + 148]
    return bits, y.astype(np.complex64)


@pytest.mark.parametrize("tsc", range(8))
def test_estimate_is_the_least_squares_fit(tsc):
    """Noise-free channel of five taps confined to the window [w0, w0 + 4]: the estimator picks w = w0 and h[k] equals the taps of a
    float64 least-squares fit over the midamble (the 22 symbols whose five contributors are all training symbols).

    Bound.  The 16 core symbols' autocorrelation is clean for shifts up to 5, so in exact arithmetic c[w0 + k] = h[k] (and the fit
    returns h, to 1e-12).  In float32, with S = sum_k |Re h[k]| + |Im h[k]| (no component of y exceeds it): the 16 inputs are
    rounded to float32, u S each, u S after the 1/16; the first addition (to 0) is exact and each of the 15 others rounds a partial
    sum of magnitude <= 16 S, 15 * 16 u S in all, 15 u S after the 1/16; the product with 0.0625 is exact.  |c - h| <= 16 u S per
    component, u = 2^-24."""
    rng = np.random.default_rng(600 + tsc)
    t = mm.tsc_symbols(tsc)
    for w0 in range(0, -5, -1):
        h = (rng.uniform(0.3, 1.0, 5) * np.exp(2j * np.pi * rng.uniform(size=5)))
        bits, y = clean_symbols(rng, tsc, h, w0)
        c, w, hh, E = mm.estimate(y, t)
        assert np.all(w == w0), (w0, w)
        a = 2.0 * bits - 1.0
        S = np.abs(h.real).sum() + np.abs(h.imag).sum()
        for b in range(len(y)):
            ms = np.arange(65 + w0, 87 + w0)                   # m - w0 - k in 61..86 for k = 0..4
            M = np.stack([a[b, ms - w0 - k] for k in range(5)], axis=1)
            fit = np.linalg.lstsq(M.astype(np.complex128), y[b, ms].astype(np.complex128), rcond=None)[0]
            assert np.abs(fit - h).max() < 1e-6                # the fit itself: y was rounded to float32
            err = np.maximum(np.abs(hh[b].real - fit.real), np.abs(hh[b].imag - fit.imag)).max()
            assert err <= 16 * U * S, (w0, b, err, 16 * U * S)


def test_one_tap_channel_gives_the_demodulators_soft_bits():
    """The trellis with the one-tap channel h = (0, 0, h0, 0, 0), w = -2, E = |h0|^2 handed in, on y = h0 a + noise (each noise
    component clipped at 0.15 |h0|): the soft bit is the demodulator's (Re(y / h0) + 1) / 2, because M_0 - M_1 = |y + h0|^2 -
    |y - h0|^2 = 4 Re(y conj(h0)) once every other branch of the two best paths is shared.  (The tap sits in the middle of the
    window so that both halves see every payload symbol: with all the energy in h[0] the left half, which reads y[m + 4 + w], never
    reads the sample that carries a[3], and with all of it in h[4] the right half never reads a[144]'s -- those two soft bits are
    then 0.5, as the algorithm is stated.)

    Bound, in units of |h0|^2 with u = 2^-24.  Expected values are +-h0 exactly.  A path sum T is at most 61 * 2 * 0.15^2 = 2.75
    of noise plus one wrong branch (2 + 0.22)^2 = 4.9: T <= 7.7.  It is built by <= 61 + 61 + 1 additions, each rounding <= 7.7 u,
    from branch metrics that carry <= 4 u relative each (two subtractions, two squares, one sum), <= 4 * 7.7 u along a path: 980 u per
    T.  M_0 - M_1 is then off by <= 2 * 980 u + 5 u, the quotient by 8 E (E exact to 3 u relative) by <= 250 u, the last addition
    adds u: |soft - demodulator's| <= 256 u = 1.5e-5 wherever the demodulator's value is not clamped.  The measured figure is printed."""
    rng = np.random.default_rng(77)
    worst = 0.0
    for tsc in (0, 5):
        h0 = np.complex64(0.8 * np.exp(2j * np.pi * rng.uniform()))
        bits, y = clean_symbols(rng, tsc, [h0], 0, n=16)
        noise = np.clip(0.05 * rng.standard_normal(y.shape), -0.15, 0.15) + 1j * np.clip(0.05 * rng.standard_normal(y.shape), -0.15, 0.15)
        y = (y + abs(h0) * noise).astype(np.complex64)
        h = np.zeros((16, 5), np.complex64); h[:, 2] = h0
        E = np.full(16, np.float32(h0.real) * np.float32(h0.real) + np.float32(h0.imag) * np.float32(h0.imag), np.float32)
        soft = mm.trellis(y, tsc, np.full(16, -2, np.int32), h, E)
        want = (np.real(y.astype(np.complex128) / np.complex128(h0)) + 1.0) / 2.0
        pay = np.r_[3:61, 87:145]
        inside = (want[:, pay] > 0.0) & (want[:, pay] < 1.0)
        assert inside.sum() > 100
        worst = max(worst, np.abs(soft[:, pay] - want[:, pay])[inside].max())
        assert np.all(soft[:, pay][want[:, pay] <= -256 * U] == 0.0) and np.all(soft[:, pay][want[:, pay] >= 1.0 + 256 * U] == 1.0)
    print("one-tap channel: max |soft - demodulator| = %.3g (%.1f u)" % (worst, worst / U))
    assert worst <= 256 * U


def test_known_symbols_are_exact():
    """Tail symbols 0..2 and 145..147 come out as exactly 0 on equalised bursts, whatever the noise."""
    n = 0
    for sps in (1, 4):
        f = mlse_family.mixed_batch(sps, 2, 67, 4100 + sps)
        eq = f["want"]["win"] <= 0
        n += int(eq.sum())
        s = f["want"]["soft"][eq]
        assert np.all(s[:, :3] == 0.0) and np.all(s[:, 145:] == 0.0)
        assert np.all((s >= 0.0) & (s <= 1.0))
    assert n > 100


def test_window_rule_is_a_strict_greater():
    """Constructed equal energies: y[62] alone makes c[-4], y[85] alone makes c[4] (no other lag reaches them), so E_0 = |c[4]|^2
    and E_-4 = |c[-4]|^2 exactly.  Equal: the first window scanned (w = 0) stays.  One ulp more in c[-4]: w = -4."""
    tsc = 3
    t = mm.tsc_symbols(tsc)
    v = np.float32(0.75)
    up = np.nextafter(v, np.float32(2.0))
    y = np.zeros((3, 148), np.complex64)
    y[0, 62] = 16.0 * t[5] * v; y[0, 85] = 16.0 * t[20] * 1j * v                    # |c[-4]| == |c[4]|
    y[1, 62] = 16.0 * t[5] * up; y[1, 85] = 16.0 * t[20] * 1j * v                   # c[-4] an ulp larger
    y[2, 62] = 16.0 * t[5] * v; y[2, 85] = 16.0 * t[20] * 1j * up                   # c[4] an ulp larger
    c, w, h, E = mm.estimate(y, t)
    assert c[0, 0] == v and c[0, 8] == 1j * v and np.count_nonzero(c[0]) == 2
    assert w.tolist() == [0, -4, 0]
    assert E[0] == v * v and E[1] == up * up
    # all nine lags equal: still w = 0
    y = np.zeros((1, 148), np.complex64)
    soft, win, h = mm.equalise(y, tsc)
    assert win[0] == mm.WIN_FELL_BACK                          # (and all-zero energies are the E == 0 fallback)


def test_fallbacks_fire():
    """length/sps < 148, a symbol component that fails fabsf(v) < 2^30 (NaN, infinity, 2^31) and E == 0: window word 1, zero taps and
    the oracle's demodulateBurst soft bits; d_enable == 0: window word 2 and zeros; the ordinary neighbours are equalised."""
    for sps in (1, 4):
        f = mlse_family.hostile_batch(sps)
        o = oraclebind.Oracle(sps)
        want = f["want"]
        for b, k in enumerate(f["kind"]):
            x = f["x"][f["off"][b]:f["off"][b] + f["length"][b]]
            if k == "plain":
                assert want["win"][b] <= 0 and np.any(want["chan"][b] != 0)
            elif k == "disabled":
                assert want["win"][b] == 2 and not want["soft"][b].any() and not want["chan"][b].any()
            else:
                assert want["win"][b] == 1 and not want["chan"][b].any(), k
                with np.errstate(all="ignore"):
                    dem = o.demodulate(x, f["amp"][b], f["toa"][b])
                n = min(148, len(x) // sps)
                same = (np.isnan(dem[:n]) & np.isnan(want["soft"][b, :n])) | (dem[:n] == want["soft"][b, :n])
                assert same.all(), k
                assert np.all(want["soft"][b, n:] == 0.5)
    # the threshold itself: 2^30 falls back, the float below it does not
    y = mlse_family.mixed_batch(1, 2, 67, 4101)["want"]["y"][:2].copy()
    y[0, 100] = np.float32(2.0 ** 30); y[1, 100] = np.nextafter(np.float32(2.0 ** 30), np.float32(0.0))
    soft, win, h = mm.equalise(y, 2)
    assert win[0] == 1 and win[1] <= 0 and np.isfinite(soft).all()


CASES = [(sps, prof) for sps in (1, 4) for prof in ("five", "precursor")]


@pytest.mark.parametrize("sps,profile", CASES)
def test_fewer_bit_errors_than_the_demodulator(sps, profile):
    """Static multipath at 15 dB, 40 bursts per case, amplitude and TOA from the oracle's analyzeTrafficBurst, payload bits
    (3..59, 88..144 and the stealing flags) of the detected bursts: the equaliser makes at most a quarter of the demodulator's
    errors.  Counted on this CPU (demodulator / equaliser, of payload bits):
        sps 1 five       277 / 0 of 3480      sps 1 precursor  101 / 0 of 4640
        sps 4 five       388 / 0 of 4060      sps 4 precursor   45 / 0 of 4640
    (the flat channel is no part of the claim: there the equaliser, estimating five taps from 16 symbols, is slightly worse)."""
    o, bits, xs, amp, toa, ok = mlse_family.static_family(sps, profile, 15.0, 40, 8800 + sps)
    sel = np.flatnonzero(ok)
    assert len(sel) >= 20
    x, off, length = mlse_family.pack(xs)
    r = mm.mlse_batch(sps, x, off[sel], length[sel], 2, amp[sel], toa[sel], oracle=o)
    dem = np.stack([o.demodulate(xs[i], amp[i], toa[i])[:148] for i in sel])
    pay = mlse_family.PAYLOAD
    e_dem = int(((dem > 0.5) != bits[sel])[:, pay].sum()); e_eq = int(((r["soft"] > 0.5) != bits[sel])[:, pay].sum())
    print("sps %d %-9s demodulator %d, equaliser %d of %d" % (sps, profile, e_dem, e_eq, len(sel) * len(pay)))
    assert e_dem >= 40 and 4 * e_eq <= e_dem
