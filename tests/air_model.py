"""The literal model of the air (include/trxsig_air.h): Philox4x32-10 in numpy integers, the Gaussian pair g in float64, and
the signal path through the oracle's primitives (convolve START_ONLY, expjLookup, delayVector, scaleVector) with every float32
operation in the order the header states.  x and the results of the cell form are lists [a][t] of complex64 arrays, t = 0 at
TN 0 of frame fn, cell t holding (156 + (t % 4 == 0)) * sps samples.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oraclebind

HYPER = 2715648
M32 = np.uint64(0xffffffff)
F32 = np.float32
TWO_PI_F = F32(2.0 * np.pi)                                     # TRX_2PI_F


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) that broadcast, key: (k0, k1) -> four uint64 arrays holding the 32-bit words"""
    c = [np.asarray(v, np.uint64) & M32 for v in np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in ctr])]
    k0, k1 = np.uint64(key[0] & 0xffffffff), np.uint64(key[1] & 0xffffffff)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                             # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def gauss(seed, i, row, plane, form):
    """g[i] of the header in float64 (complex128): i an array of sample indices (uint32 range)"""
    i = np.asarray(i, np.uint64) & M32
    w = philox4x32_10((i >> np.uint64(1), row, plane, form), (seed & 0xffffffff, seed >> 32))
    odd = (i & np.uint64(1)).astype(bool)
    wa, wb = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
    u = (2.0 * (wa >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    v = (2.0 * (wb >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u))
    return r * np.cos(2.0 * np.pi * v) + 1j * r * np.sin(2.0 * np.pi * v)


def cell_len(t, sps):
    return (156 + (t % 4 == 0)) * sps


def cell_gauss(seed, fn, t, a, n):
    """the cell form's g for the n samples of slot t (from frame fn) of ARFCN a"""
    return gauss(seed, np.arange(n), (8 * fn + t) % (8 * HYPER), a, 0)


def stream_gauss(seed, h, n0, n):
    return gauss(seed, (int(n0) + np.arange(n, dtype=np.uint64)) & M32, h, 0, 1)


def cmul32(x, a):
    """Complex<float>::operator*: (x.r a.r - x.i a.i, x.r a.i + x.i a.r), every product and sum rounded to float32"""
    x, a = np.asarray(x, np.complex64), np.asarray(a, np.complex64)
    xr, xi, ar, ai = x.real.astype(F32), x.imag.astype(F32), a.real.astype(F32), a.imag.astype(F32)
    out = np.empty(np.broadcast(x, a).shape, np.complex64)
    with np.errstate(all="ignore"):
        out.real = xr * ar - xi * ai
        out.imag = xr * ai + xi * ar
    return out


class AirModel:
    def __init__(self, o):
        self.o, self.sps = o, o.sps
        self._e = {}

    def rot(self, phase, step, n):
        """expjLookup((float)(p_i >> 8) * 2^-24f * (float)(2 pi)), p_i = phase + i step mod 2^32, i < n"""
        p = (int(phase) + np.arange(n, dtype=np.uint64) * np.uint64(int(step))) & M32
        top = (p >> np.uint64(8)).astype(np.int64)
        for v in np.unique(top):
            if int(v) not in self._e:
                self._e[int(v)] = np.complex64(self.o.expjLookup(F32(v) * F32(2.0 ** -24) * TWO_PI_F))
        return np.array([self._e[int(v)] for v in top], np.complex64)

    def signal(self, x, h=None, step=None, phase=0):
        """stages 1 and 2 on one cell"""
        u = np.asarray(x, np.complex64)
        if h is not None:
            u = self.o.convolve(u, np.asarray(h, np.complex64), oraclebind.START_ONLY)
        if step is not None:
            u = cmul32(u, self.rot(phase, step, len(u)))
        return u

    def cells(self, fn, x, seed=0, taps=None, step=None, phase=None, sigma=None, base=None):
        """The cell form.  taps [a][t][Lh] / step, phase, sigma [a][t] or None; base: the buffer accumulated onto (accumulate != 0)
        or None.  With sigma the noise is the float64 g rounded once into the float32 sum (not the device's words)."""
        out = []
        for a, row in enumerate(x):
            out.append([])
            for t, c in enumerate(row):
                assert len(c) == cell_len(t, self.sps)
                w = self.signal(c, None if taps is None else taps[a][t], None if step is None else step[a][t],
                                0 if phase is None else phase[a][t])
                if sigma is not None:
                    w = (w.astype(np.complex128) + float(F32(sigma[a][t])) * cell_gauss(seed, fn, t, a, len(c))).astype(np.complex64)
                if base is not None:
                    with np.errstate(all="ignore"):
                        w = (np.asarray(base[a][t], np.complex64) + w).astype(np.complex64)
                out[-1].append(w)
        return out

    def stream(self, x, seed, arfcn, cut, length, delay=None, step=None, phase=None, gain=None, sigma=None, n0=None):
        """The stream form: per-handset lists (or None: the stage is skipped) -> [n_handsets][length] complex64"""
        out = np.zeros((len(arfcn), length), np.complex64)
        for h, a in enumerate(arfcn):
            c = np.concatenate(x[a]).astype(np.complex64)
            z = c if delay is None else self.o.delay_vector(c, F32(delay[h]))
            k = int(cut[h]) + np.arange(length)
            ok = (k >= 0) & (k < len(z))
            y = np.zeros(length, np.complex64)
            y[ok] = z[k[ok]]
            if step is not None:
                y = cmul32(y, self.rot(0 if phase is None else phase[h], step[h], length))
            if gain is not None:
                y = self.o.scale_vector(y, np.complex64(gain[h]))
            if sigma is not None:
                g = stream_gauss(seed, h, 0 if n0 is None else n0[h], length)
                y = (y.astype(np.complex128) + float(F32(sigma[h])) * g).astype(np.complex64)
            out[h] = y
        return out


def random_cells(rng, n_arfcn, n_slots, sps, amp=1.0):
    return [[(amp * (rng.standard_normal(cell_len(t, sps)) + 1j * rng.standard_normal(cell_len(t, sps)))).astype(np.complex64)
             for t in range(n_slots)] for _ in range(n_arfcn)]
