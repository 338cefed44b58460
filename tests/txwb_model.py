"""The wideband transmit synthesiser (include/trxsig_frontend.h, trxsig_txbe_create_wideband) composed from the CPU oracle's
primitives, as the header's numerical contract states it: per ARFCN stream modulateBurst (x gain) behind a 130 sps zero history,
polyphaseResampleVector(P = 96 R, Q = 65 sps) per whole chunks with the first 192 R outputs dropped; per wideband stream the
channeliser's mixer (Oracle.mix_down at the emitted-sample count, frequency -f_c), a carrier-order complex64 sum from 0,
scaleVector(gain), truncation and the int16 clip."""
import numpy as np


class TxwbModel:
    def __init__(self, o, n_wide, carrier_freq, rate_factor, lpf, gain):
        self.o, self.sps = o, o.sps
        self.Sw, self.f = n_wide, np.float32(carrier_freq).ravel()
        self.C, self.R = self.f.size, rate_factor
        self.lpf, self.gain = np.float32(lpf), np.float32(gain)
        self.S = self.Sw * self.C
        self.Q = 65 * self.sps
        self.inchunk = 9 * self.Q
        self.hist = [np.zeros(2 * self.Q, np.complex64) for _ in range(self.S)]
        self.send = [np.zeros(0, np.complex64) for _ in range(self.S)]
        self.k = 0                                          # int16 samples emitted per wideband stream

    def push(self, bits, guard, gain=None):
        """bits [S, nb, 148], guard [nb], gain [S, nb] or None: modulateBurst (x gain) appended to every ARFCN stream."""
        for s in range(self.S):
            xs = []
            for j in range(bits.shape[1]):
                x = self.o.modulate(bits[s, j].astype(np.int8), int(guard[j]))
                if gain is not None:
                    x = self.o.scale_vector(x, complex(gain[s, j], 0.0))
                xs.append(x)
            self.send[s] = np.concatenate([self.send[s]] + xs)

    def resampled(self, nch):
        """y_s for the next nch chunks of every ARFCN stream (moves the history on)."""
        P, R = 96 * self.R, self.R
        ys = []
        for s in range(self.S):
            tr = self.send[s][:nch * self.inchunk]
            y = self.o.polyphase_resample(np.concatenate([self.hist[s], tr]), P, self.Q, self.lpf)
            ys.append(y[192 * R:192 * R + 864 * R * nch])
            self.hist[s] = tr[-2 * self.Q:]
            self.send[s] = self.send[s][nch * self.inchunk:]
        return ys

    def pop(self, clip=True):
        """int16 [Sw, 864 R nch, 2] (I first), or None while less than one chunk is buffered."""
        nch = len(self.send[0]) // self.inchunk
        if nch == 0:
            return None
        ys = self.resampled(nch)
        n = 864 * self.R * nch
        out = np.zeros((self.Sw, n, 2), np.int16)
        self.peak = 0.0                                     # the largest |component| before the clip
        for w in range(self.Sw):
            z = np.zeros(n, np.complex64)
            for c in range(self.C):
                z = z + self.o.mix_down(ys[w * self.C + c], self.k, np.float32(-self.f[c]))
            v = self.o.scale_vector(z, complex(float(self.gain), 0.0))
            re, im = np.trunc(v.real.astype(np.float64)), np.trunc(v.imag.astype(np.float64))
            self.peak = max(self.peak, float(np.abs(re).max()), float(np.abs(im).max()))
            if clip:
                re, im = np.clip(re, -32768, 32767), np.clip(im, -32768, 32767)
            out[w, :, 0] = re.astype(np.int64).astype(np.int16)
            out[w, :, 1] = im.astype(np.int64).astype(np.int16)
        self.k += n
        return out

