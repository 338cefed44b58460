"""A float64 reference of the multi-ARFCN channeliser (trxsig_rxfe_create_wideband / push_wideband), written from the
definition rather than from either kernel: int16 I/Q -> complex, the zero history of 192 x CW raw samples in front of the
stream, windows of history + 864 x CW samples per chunk, and per window the polyphase sum

    y_c[o] = sum_k h[branch + P k] * x[n - k] * exp(j theta_c (n - k)),   n = floor((o + D) Q / P),  branch = (o + D) Q mod P,

D = (L - 1) / 2 / Q, taps outside the filter or the window skipped, then pullBuffer's skip of 2 P outputs per window.  The
phase index n - k counts raw samples from the first history sample (the front end's convention: the stream's first sample
is raw sample 192 x CW).  Every output comes with A(o) = sum_k |h_k| (|Re x| + |Im x|), the scale a float32 evaluation's
rounding error is proportional to.  Plain numpy, no GPU; tests/test_chan_ref.py pins it on the reference's own primitives."""
import math

import numpy as np

OUTRATE, OUTCHUNK, OUTHISTORY = 96, 864, 192
U = 2.0 ** -24                                       # float32 unit roundoff


def geometry(sps, cw):
    """(P, Q, chunk, hist, skip, n_out) of a wideband front end: n_out = ceil(n * (float) P / (float) Q) per window
    (sigProcLib.cpp:1171, float arithmetic), of which the first skip = 2 P are dropped."""
    P, Q = 65 * sps, OUTRATE * cw
    chunk, hist = OUTCHUNK * cw, OUTHISTORY * cw
    n_out = int(math.ceil(float(np.float32(hist + chunk) * np.float32(P) / np.float32(Q))))
    return P, Q, chunk, hist, 2 * P, n_out


def to_complex(iq, swap_iq=True):
    """int16 [n, 2] -> complex128: with swap_iq the radio's pairs are (Q, I) (unUSRPifyVector's order)."""
    iq = np.asarray(iq)
    re, im = (iq[:, 1], iq[:, 0]) if swap_iq else (iq[:, 0], iq[:, 1])
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def grid_mixer(bins):
    """exp(j 2 pi b n / 16) for every bin b, evaluated exactly on the grid (n reduced mod 16 in integers first)."""
    bins = [int(b) for b in bins]

    def mix(c, n):
        return np.exp(2j * np.pi * ((bins[c] * n) % 16) / 16.0)
    return mix, len(bins)


def theta_mixer(theta):
    """exp(j theta_c n) for arbitrary theta (float64; e.g. a float32 carrier frequency widened)."""
    theta = [float(t) for t in theta]

    def mix(c, n):
        return np.exp(1j * (theta[c] * n.astype(np.float64)))
    return mix, len(theta)


def table_mixer(table):
    """Mixer values given explicitly: table[c][n] for raw sample n (counted from the first history sample)."""
    table = np.asarray(table)

    def mix(c, n):
        return table[c][n].astype(np.complex128)
    return mix, table.shape[0]


def channelise(iq, sps, cw, lpf, mixer, swap_iq=True):
    """iq: int16 [n_chunks * 864 * cw, 2], one wideband stream; mixer: (mix, C) from grid_mixer / theta_mixer / table_mixer;
    lpf: the L taps (float32 values, used widened).  Returns y complex128 [C, n_chunks * (n_out - 2 P)] and A float64
    [n_chunks * (n_out - 2 P)] (A does not depend on the carrier: |exp(j phi)| = 1)."""
    mix, C = mixer
    P, Q, chunk, hist, skip, n_out = geometry(sps, cw)
    h = np.asarray(lpf, np.float32).astype(np.float64)
    L = h.size
    D = (L - 1) // 2 // Q
    x = to_complex(iq, swap_iq)
    assert x.size % chunk == 0
    n_chunks = x.size // chunk
    n_win = hist + chunk
    oi = np.arange(skip, n_out, dtype=np.int64) + D
    branch = (oi * Q) % P
    in_off = (oi * Q) // P
    K = (L + P - 1) // P
    k = np.arange(K, dtype=np.int64)
    idx = in_off[:, None] - k[None, :]                      # window sample met by tap k
    fi = branch[:, None] + P * k[None, :]                   # its filter index
    valid = (fi < L) & (idx >= 0) & (idx < n_win)
    hv = np.where(valid, h[np.minimum(fi, L - 1)], 0.0)
    idc = np.clip(idx, 0, n_win - 1)
    ys, As = [[] for _ in range(C)], []
    prev = np.zeros(hist, np.complex128)                    # rcvHistory->fill(0)
    for c in range(n_chunks):
        win = np.concatenate([prev, x[c * chunk:(c + 1) * chunk]])
        xv = np.where(valid, win[idc], 0.0)
        hx = hv * xv
        As.append((np.abs(hv) * (np.abs(xv.real) + np.abs(xv.imag))).sum(axis=1))
        nglob = c * chunk + idc                             # raw index from the first history sample
        for car in range(C):
            ys[car].append((hx * mix(car, nglob)).sum(axis=1))
        prev = win[-hist:]
    return np.stack([np.concatenate(v) for v in ys]), np.concatenate(As)
