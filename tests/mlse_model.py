"""The float32 model of the sequence equaliser (trxsig_mlse_batch, csrc/trxsig_mlse.hip): the algorithm of include/trxsig.h
restated in numpy float32, operation by operation, vectorised over bursts.  The kernel must equal it word for word.

Every arithmetic step below is ONE float32 operation on float32 arrays (numpy rounds each separately; nothing here is a
float64 intermediate), in the order the header states.  The symbols come from the CPU oracle's scale_vector / delay_vector /
gmsk_rotate with the reference's 1/amp (cinv, then the product with (1, 0)).
"""
import numpy as np

import oraclebind
import synth

F = np.float32
INF = F(np.inf)
WIN_FELL_BACK, WIN_SKIPPED = 1, 2


def tsc_symbols(tsc):
    """t[j] = a[61 + j] = 2 bit - 1, float32 [26]."""
    return (2.0 * np.array([int(ch) for ch in synth.TRAINING_SEQUENCE[tsc]], np.float32) - 1.0).astype(F)


def inv_amp(amp):
    """((complex)1.0) / amp as Complex.h forms it: cinv (n = i*i + r*r; (r/n, -i/n)), then (1, 0) * that."""
    a = np.complex64(amp)
    with np.errstate(all="ignore"):
        r, i = F(a.real), F(a.imag)
        n = F(F(i * i) + F(r * r))
        cr, ci = F(r / n), F(F(-i) / n)
        one, zero = F(1.0), F(0.0)
        return F(F(one * cr) - F(zero * ci)), F(F(one * ci) + F(zero * cr))


def burst_enabled(sps, off, n, toa):
    """k_demod's own test of a burst's geometry (a NaN TOA fails it)."""
    with np.errstate(all="ignore"):
        return bool(off >= 0 and 92 * sps <= n <= 157 * sps and n % sps == 0 and np.abs(F(toa)) <= F(4096.0))


def symbols(oracle, x, amp, toa):
    """y[0..147]: demodulateBurst's vector just before vectorSlicer, both parts (zeros past a short burst's end)."""
    sps = oracle.sps
    ir, ii = inv_amp(amp)
    with np.errstate(all="ignore"):
        d = oracle.scale_vector(np.ascontiguousarray(x, np.complex64), complex(ir, ii))
        d = oracle.delay_vector(d, F(-F(toa)))
        d = oracle.gmsk_rotate(d, reverse=True)
    y = np.zeros(148, np.complex64)
    ns = min(148, len(x) // sps)
    y[:ns] = d[::sps][:ns]
    return y


def slicer(re):
    """vectorSlicer on a symbol's real part: clamp((re + 1) * 0.5) with the demodulator's comparisons (a NaN stays a NaN)."""
    with np.errstate(all="ignore"):
        sv = ((re.astype(F) + F(1.0)) * F(0.5)).astype(F)
        sv = np.where(sv > F(1.0), F(1.0), sv)
        sv = np.where(sv < F(0.0), F(0.0), sv)
    return sv.astype(F)


def estimate(y, t):
    """Step 2 on symbols y [B, 148] (complex64) with training symbols t [26]: (c [B, 9] for d = -4..4, w [B], h [B, 5], E [B])."""
    B = y.shape[0]
    yr, yi = y.real.astype(F), y.imag.astype(F)
    cr = np.zeros((B, 9), F); ci = np.zeros((B, 9), F)
    for k, d in enumerate(range(-4, 5)):
        ar = np.zeros(B, F); ai = np.zeros(B, F)
        for i in range(16):
            ar = ar + t[5 + i] * yr[:, 66 + i + d]            # the sign flip is exact
            ai = ai + t[5 + i] * yi[:, 66 + i + d]
        cr[:, k] = F(0.0625) * ar; ci[:, k] = F(0.0625) * ai
    p = cr * cr + ci * ci

    def energy(w):
        k = w + 4
        return (((p[:, k] + p[:, k + 1]) + p[:, k + 2]) + p[:, k + 3]) + p[:, k + 4]
    E = energy(0); w = np.zeros(B, np.int32)
    for q in range(1, 5):
        Ew = energy(-q)
        take = Ew > E                                          # a later window only on a strict >
        E = np.where(take, Ew, E); w = np.where(take, -q, w).astype(np.int32)
    idx = (w + 4)[:, None] + np.arange(5)[None, :]
    rows = np.arange(B)[:, None]
    h = (cr[rows, idx] + 1j * ci[rows, idx]).astype(np.complex64)
    return (cr + 1j * ci).astype(np.complex64), w, h, E.astype(F)


def _half(yr, yi, w, gr, gi, start, left):
    """One half-burst trellis for every burst: M_0 - M_1 per step, [B, 61].  yr, yi [B, 148]; gr, gi [B, 5]; start [B]."""
    B = yr.shape[0]
    x = np.arange(32)
    sign = np.where(((x[:, None] >> np.arange(5)[None, :]) & 1) == 1, F(1.0), F(-1.0)).astype(F)     # [32, 5]
    Zr = gr[:, None, 0] * sign[None, :, 0]; Zi = gi[:, None, 0] * sign[None, :, 0]
    for k in range(1, 5):
        Zr = Zr + gr[:, None, k] * sign[None, :, k]
        Zi = Zi + gi[:, None, k] * sign[None, :, k]
    rows = np.arange(B)
    gam = np.zeros((61, B, 32), F)
    for i in range(61):
        n = (60 - i + 4 + w) if left else (87 + i + w)
        dr = yr[rows, n][:, None] - Zr; di = yi[rows, n][:, None] - Zi
        g = dr * dr + di * di
        if i >= 58:
            g[:, 1::2] = INF                                   # the tail symbols are -1: b = 1 contradicts
        gam[i] = g
    s = np.arange(16)
    alpha = np.where(s[None, :] == start[:, None], F(0.0), INF).astype(F)
    A = np.zeros((61, B, 16), F)
    p0, p1 = s >> 1, (s >> 1) | 8
    for i in range(61):
        alpha = np.minimum(alpha[:, p0] + gam[i][:, s], alpha[:, p1] + gam[i][:, s | 16])     # x = (pred << 1) | b
        A[i] = alpha
    beta = np.zeros((B, 16), F)
    D = np.zeros((B, 61), F)
    for i in range(60, -1, -1):
        T = A[i] + beta
        D[:, i] = T[:, 0::2].min(axis=1) - T[:, 1::2].min(axis=1)
        x0, x1 = 2 * s, 2 * s + 1
        beta = np.minimum(gam[i][:, x0] + beta[:, x0 & 15], gam[i][:, x1] + beta[:, x1 & 15])
    return D


def trellis(y, tsc, w, h, E):
    """Steps 3-4 on symbols y [B, 148] with given windows w [B], taps h [B, 5] and energies E [B]: soft [B, 148] float32 (the
    demodulator's formula on 61..86)."""
    y = np.ascontiguousarray(y, np.complex64)
    B = y.shape[0]
    t = tsc_symbols(tsc)
    yr, yi = y.real.astype(F), y.imag.astype(F)
    hr, hi = h.real.astype(F), h.imag.astype(F)
    bit = (t > 0).astype(np.int64)
    start_r = np.full(B, bit[25] | (bit[24] << 1) | (bit[23] << 2) | (bit[22] << 3))
    start_l = np.full(B, bit[0] | (bit[1] << 1) | (bit[2] << 2) | (bit[3] << 3))
    with np.errstate(all="ignore"):
        Dr = _half(yr, yi, w, hr, hi, start_r, False)
        Dl = _half(yr, yi, w, hr[:, ::-1], hi[:, ::-1], start_l, True)
        den = (F(8.0) * E.astype(F))[:, None]
        sr = F(0.5) + Dr / den
        sl = F(0.5) + Dl / den
        sr = np.where(sr > F(1.0), F(1.0), sr); sr = np.where(sr < F(0.0), F(0.0), sr)
        sl = np.where(sl > F(1.0), F(1.0), sl); sl = np.where(sl < F(0.0), F(0.0), sl)
    soft = slicer(yr)
    soft[:, 87:148] = sr
    soft[:, 60::-1] = sl                                      # step i is symbol 60 - i
    return soft.astype(F)


def equalise(y, tsc):
    """Steps 2-5 on symbols y [B, 148]: (soft [B, 148] float32, win [B] int32 (w, or 1 = fell back), h [B, 5] complex64 (zeros on fallback))."""
    y = np.ascontiguousarray(y, np.complex64)
    t = tsc_symbols(tsc)
    with np.errstate(all="ignore"):
        fine = (np.abs(y.real) < F(2.0 ** 30)).all(axis=1) & (np.abs(y.imag) < F(2.0 ** 30)).all(axis=1)
        ys = np.where(fine[:, None], y, 0).astype(np.complex64)     # (a burst that falls back runs through below on zeros, unused)
        _, w, h, E = estimate(ys, t)
        ok = fine & (E != 0)
        eq = trellis(ys, tsc, w, h, E)
    soft = np.where(ok[:, None], eq, slicer(y.real.astype(F))).astype(F)
    win = np.where(ok, w, WIN_FELL_BACK).astype(np.int32)
    h = np.where(ok[:, None], h, 0).astype(np.complex64)
    return soft, win, h


def mlse_batch(sps, x, off, length, tsc, amp, toa, enable=None, nsoft=148, oracle=None):
    """trxsig_mlse_batch on packed bursts: dict(soft [B, nsoft], hard, win [B], chan [B, 5], y [B, 148])."""
    o = oracle or oraclebind.Oracle(sps)
    B = len(off)
    amp = np.broadcast_to(np.asarray(amp, np.complex64), (B,)); toa = np.broadcast_to(np.asarray(toa, np.float32), (B,))
    y = np.zeros((B, 148), np.complex64)
    state = np.zeros(B, np.int32)
    for b in range(B):
        if (enable is not None and not enable[b]) or not burst_enabled(sps, int(off[b]), int(length[b]), toa[b]):
            state[b] = WIN_SKIPPED
            continue
        y[b] = symbols(o, x[off[b]:off[b] + length[b]], amp[b], toa[b])
        if length[b] // sps < 148:
            state[b] = WIN_FELL_BACK
    soft, win, h = equalise(y, tsc)
    short = state == WIN_FELL_BACK
    if short.any():
        soft[short] = slicer(y[short].real)
        win[short] = WIN_FELL_BACK; h[short] = 0
    skip = state == WIN_SKIPPED
    soft[skip] = 0; win[skip] = WIN_SKIPPED; h[skip] = 0
    soft = np.ascontiguousarray(soft[:, :nsoft])
    with np.errstate(all="ignore"):
        hard = (soft > F(0.5)).astype(np.uint8)
    return dict(soft=soft, hard=hard, win=win, chan=h, y=y)
