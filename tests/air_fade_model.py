"""The model of the fading-tap generator (include/trxsig_air.h, "Time-varying multipath"): the integers (phi, C, step, the column
rotations) word for word -- Philox4x32-10 from air_model, the float32 trig steps restated in numpy float32 -- and the taps in
float64 from those integers.  The library has no counterpart in the reference (a base station does not simulate its own
propagation): this file is the definition the device is held to.  TEST INFRASTRUCTURE ONLY.

The PROFILES below are written from memory in the style of GSM 05.05 annex C (typical urban, rural area, hilly terrain, the
equaliser test).  They are inputs that give the tests and the bench realistic shapes, not a contract: nothing checks them against
the specification and the library holds no such table."""
import numpy as np

import air_model as am

F32 = np.float32
ROWS = 8 * am.HYPER
D_TRIG = 1e-5                                                   # the header's promise for each component of e
U = 2.0 ** -24

# name -> (delays in ns, powers in dB, line-of-sight share of path 0, its arrival cosine in Q23)
PROFILES = {
    "TU6": ([0, 200, 500, 1600, 2300, 5000], [-3.0, 0.0, -2.0, -6.0, -8.0, -10.0], 0.0, 0),
    "RA6": ([0, 100, 200, 300, 400, 500], [0.0, -4.0, -8.0, -12.0, -16.0, -20.0], 0.5, int(0.7 * 2 ** 23)),
    "HT6": ([0, 100, 300, 500, 15000, 17200], [0.0, -1.5, -4.5, -7.5, -8.0, -17.7], 0.0, 0),
    "EQ6": ([0, 3200, 6400, 9600, 12800, 16000], [0.0] * 6, 0.0, 0),
}


def profile(name):
    """-> dict(delay_ns, power (normalised to a sum of 1), los_share, los_cos_q23) of a named profile"""
    d, db, los, lc = PROFILES[name]
    p = 10.0 ** (np.asarray(db) / 10.0)
    ls, c = np.zeros(len(d), np.float32), np.zeros(len(d), np.int32)
    ls[0], c[0] = los, lc
    return dict(delay_ns=np.asarray(d, np.int32), power=(p / p.sum()).astype(np.float32), los_share=ls, los_cos_q23=c)


def cossin24(k):
    """(cos, sin) of the 24-bit phase k (2^-24 turn) by the device's float32 steps: octant reduction in integers, one rounded
    product for the angle, Taylor polynomials in Horner form with every operation rounded to float32"""
    k = np.asarray(k, np.int64) & 0xffffff
    quad = k >> 22
    f = k & 0x3fffff
    mirror = f > 0x200000
    f = np.where(mirror, 0x400000 - f, f)
    th = f.astype(F32) * F32(3.74507028e-7)
    t2 = th * th
    ps = t2 * F32(2.75573192e-6) + F32(-1.98412698e-4)
    ps = ps * t2 + F32(8.33333333e-3)
    ps = ps * t2 + F32(-0.166666667)
    ps = ps * t2
    sn = th + th * ps
    pc = t2 * F32(-2.75573192e-7) + F32(2.48015873e-5)
    pc = pc * t2 + F32(-1.38888889e-3)
    pc = pc * t2 + F32(4.16666667e-2)
    pc = pc * t2 + F32(-0.5)
    cs = F32(1.0) + pc * t2
    assert sn.dtype == F32 and cs.dtype == F32
    sn, cs = np.where(mirror, cs, sn), np.where(mirror, sn, cs)
    c = np.select([quad == 0, quad == 1, quad == 2], [cs, -sn, -cs], sn)
    s = np.select([quad == 0, quad == 1, quad == 2], [sn, cs, -sn], -cs)
    return c.astype(F32), s.astype(F32)


def rot_phase(khz, ns):
    """-f_kHz tau_ns 1e-6 turn in 2^-32 turn, in Python integers: whole turns dropped, one rounding, halves up"""
    r = (-int(khz) * int(ns)) % 1000000
    return ((r << 32) + 500000) // 1000000 & 0xffffffff


def weights(delay_ns, sps, n_taps, centre):
    """w[p][j] float32: the Hann-windowed sinc of half-width 4 samples centred at centre + tau_p samples"""
    w = np.zeros((len(delay_ns), n_taps), np.float64)
    for p, ns in enumerate(delay_ns):
        at = 48000 * centre + 13 * sps * int(ns)
        for j in range(n_taps):
            num = 48000 * j - at
            if num % 48000 == 0:
                w[p, j] = 1.0 if num == 0 else 0.0
            elif abs(num) < 4 * 48000:
                x = num / 48000.0
                w[p, j] = np.sin(np.pi * x) / (np.pi * x) * (0.5 + 0.5 * np.cos(np.pi * x / 4.0))
    return w.astype(F32)


class FadeModel:
    def __init__(self, sps, delay_ns, power, n_sinusoids, n_taps, centre=0, los_share=None, los_cos_q23=None, col_khz=None):
        self.sps, self.S, self.n_taps, self.centre = sps, int(n_sinusoids), int(n_taps), int(centre)
        self.delay_ns = np.asarray(delay_ns, np.int32)
        self.P = len(self.delay_ns)
        pw = np.asarray(power, np.float32).astype(np.float64)
        los = np.zeros(self.P) if los_share is None else np.asarray(los_share, np.float32).astype(np.float64)
        self.los_c = np.zeros(self.P, np.int64) if los_cos_q23 is None else np.asarray(los_cos_q23, np.int64)
        self.a = np.sqrt(pw * (1.0 - los) / self.S).astype(F32)
        self.b = np.sqrt(pw * los).astype(F32)
        self.w = weights(self.delay_ns, sps, self.n_taps, self.centre)
        self.col_khz = [200 * a for a in range(1024)] if col_khz is None else [int(v) for v in col_khz]

    def cosines(self, seed, n_links):
        """-> phi (uint32), C (int64, Q23), both [n_links][P][S + 1]"""
        S, P = self.S, self.P
        s = np.arange(S + 1, dtype=np.uint64)[None, None, :]
        p = np.arange(P, dtype=np.uint64)[None, :, None]
        l = np.arange(n_links, dtype=np.uint64)[:, None, None]
        w = am.philox4x32_10((s, p, l, 2), (seed & 0xffffffff, seed >> 32))
        c, _ = cossin24(2 * (w[1] >> np.uint64(9)).astype(np.int64) + 1)
        C = np.rint(c * F32(8388608.0)).astype(np.int64)        # (ties to even, as rintf)
        C[:, :, S] = self.los_c[None, :]
        return w[0].astype(np.uint32), C

    def params(self, seed, n_links, doppler):
        """-> phi (uint32), step (int32), both [n_links][P][S + 1]: the words trxsig_air_fade_params writes"""
        phi, C = self.cosines(seed, n_links)
        D = (np.asarray(doppler, np.uint32).astype(np.int64) & 0x7fffffff)[:n_links, None, None]
        step = (C * D) >> 23                                    # numpy's >> on int64 is arithmetic: towards minus infinity
        assert (np.abs(step) < 2 ** 31).all()
        return phi, step.astype(np.int32)

    def rot(self, a):
        return np.array([rot_phase(self.col_khz[a], ns) for ns in self.delay_ns], np.int64)

    @staticmethod
    def theta(phi, step, row):
        """phi + row step mod 2^32: [..links..][len(row)][P][S + 1] (int64 holds row * step: below 2^25 * 2^31)"""
        row = np.asarray(row, np.int64)[:, None, None]
        return (phi.astype(np.int64)[..., None, :, :] + row * step.astype(np.int64)[..., None, :, :]) & 0xffffffff

    def gains(self, phi, step, row, a):
        """g_p rotated for column a at the rows given: complex128 [..links..][len(row)][P] from the integers phi, step
        [..links..][P][S + 1]; the trig is float64 of the 24-bit phases the device evaluates"""
        e = np.exp(2j * np.pi * (self.theta(phi, step, row) >> 8) * 2.0 ** -24)
        g = self.a.astype(np.float64) * e[..., :self.S].sum(axis=-1) + self.b.astype(np.float64) * e[..., self.S]
        return g * np.exp(2j * np.pi * (self.rot(a) >> 8) * 2.0 ** -24)

    def taps(self, fn, n_arfcn, n_frames, seed, n_links, doppler, link=None):
        """-> complex128 [n_arfcn][8 n_frames][n_taps]: the float64 value of what trxsig_air_fade writes"""
        T = 8 * n_frames
        phi, step = self.params(seed, n_links, doppler)
        t = np.arange(T)
        rows = (8 * fn + t) % ROWS
        out = np.zeros((n_arfcn, T, self.n_taps), np.complex128)
        for a in range(n_arfcn):
            l = 8 * a + t % 8 if link is None else np.asarray(link[a], np.int64)
            ok = (l >= 0) & (l < n_links)
            g = self.gains(phi, step, rows, a)
            h = sum(g[..., p, None] * self.w[p].astype(np.float64) for p in range(self.P))   # [n_links][T][n_taps], p ascending
            out[a, ok] = h[l[ok], t[ok]]
        return out

    def bound(self):
        """The header's error bound per component of tap[j]: float64 [n_taps]"""
        S, P = self.S, self.P
        a, b, w = self.a.astype(np.float64), self.b.astype(np.float64), np.abs(self.w.astype(np.float64))
        G = S * a + b
        E = a * (S * D_TRIG + S * S * U) + b * D_TRIG + 3 * U * G
        R = 2 * E + 2 * G * D_TRIG + 6 * U * G
        return (w * (R + 2 * G * (2 * U + (P + 1) * U))[:, None]).sum(axis=0)
