"""The float32 model of the two-antenna sequence equaliser (trxsig_mlse_div_batch, csrc/trxsig_mlse_div.hip): the algorithm of
include/trxsig.h restated in numpy float32, operation by operation, vectorised over bursts.  The kernel must equal it word for
word.  It is tests/mlse_model.py with a second antenna: the symbols, the slicer, the training symbols, 1/amp and the geometry test
are that module's; the estimator, the two half-burst trellises and the fallbacks are stated again here, with the tap powers and
the branch metrics summed over the antennas (antenna 0's term first, one float32 addition).

Every arithmetic step below is ONE float32 operation on float32 arrays, in the order the header states."""
import numpy as np

import oraclebind
from mlse_model import burst_enabled, inv_amp, slicer, symbols, tsc_symbols  # noqa: F401  (inv_amp: what symbols() scales by)

F = np.float32
INF = F(np.inf)
WIN_FELL_BACK, WIN_SKIPPED = 1, 2


def correlate(y, t):
    """c[d], d = -4..4, of one antenna's symbols y [B, 148]: (re, im) [B, 9] float32."""
    B = y.shape[0]
    yr, yi = y.real.astype(F), y.imag.astype(F)
    cr = np.zeros((B, 9), F); ci = np.zeros((B, 9), F)
    for k, d in enumerate(range(-4, 5)):
        ar = np.zeros(B, F); ai = np.zeros(B, F)
        for i in range(16):
            ar = ar + t[5 + i] * yr[:, 66 + i + d]            # the sign flip is exact
            ai = ai + t[5 + i] * yi[:, 66 + i + d]
        cr[:, k] = F(0.0625) * ar; ci[:, k] = F(0.0625) * ai
    return cr, ci


def estimate(y, t):
    """Step 2 on symbols y [B, 2, 148] (complex64) with training symbols t [26]: (c [B, 2, 9] for d = -4..4, w [B], h [B, 2, 5], E [B])."""
    B = y.shape[0]
    c0r, c0i = correlate(y[:, 0], t)
    c1r, c1i = correlate(y[:, 1], t)
    p = (c0r * c0r + c0i * c0i) + (c1r * c1r + c1i * c1i)

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
    c = np.stack([c0r + 1j * c0i, c1r + 1j * c1i], axis=1).astype(np.complex64)
    h = np.stack([c[:, 0][rows, idx], c[:, 1][rows, idx]], axis=1).astype(np.complex64)      # one window for both antennas
    return c, w, h, E.astype(F)


def _expected(gr, gi):
    """Z[x], x = 0..31, of taps g [B, 5]: (re, im) [B, 32]; starts from +-g[0], adds k = 1..4 in order."""
    x = np.arange(32)
    sign = np.where(((x[:, None] >> np.arange(5)[None, :]) & 1) == 1, F(1.0), F(-1.0)).astype(F)     # [32, 5]
    Zr = gr[:, None, 0] * sign[None, :, 0]; Zi = gi[:, None, 0] * sign[None, :, 0]
    for k in range(1, 5):
        Zr = Zr + gr[:, None, k] * sign[None, :, k]
        Zi = Zi + gi[:, None, k] * sign[None, :, k]
    return Zr, Zi


def _half(yr, yi, w, gr, gi, start, left):
    """One half-burst trellis for every burst: M_0 - M_1 per step, [B, 61].  yr, yi [B, 2, 148]; gr, gi [B, 2, 5]; start [B]."""
    B = yr.shape[0]
    Z0r, Z0i = _expected(gr[:, 0], gi[:, 0])
    Z1r, Z1i = _expected(gr[:, 1], gi[:, 1])
    rows = np.arange(B)
    gam = np.zeros((61, B, 32), F)
    for i in range(61):
        n = (60 - i + 4 + w) if left else (87 + i + w)
        dr0 = yr[rows, 0, n][:, None] - Z0r; di0 = yi[rows, 0, n][:, None] - Z0i
        dr1 = yr[rows, 1, n][:, None] - Z1r; di1 = yi[rows, 1, n][:, None] - Z1i
        g = (dr0 * dr0 + di0 * di0) + (dr1 * dr1 + di1 * di1)
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


def trellis(y, tsc, w, h, E, primary=None):
    """Steps 3-4 on symbols y [B, 2, 148] with given windows w [B], taps h [B, 2, 5] and energies E [B]: soft [B, 148] float32 (the
    demodulator's formula on the primary antenna on 61..86)."""
    y = np.ascontiguousarray(y, np.complex64)
    B = y.shape[0]
    primary = np.zeros(B, np.int64) if primary is None else np.asarray(primary, np.int64)
    t = tsc_symbols(tsc)
    yr, yi = y.real.astype(F), y.imag.astype(F)
    hr, hi = h.real.astype(F), h.imag.astype(F)
    bit = (t > 0).astype(np.int64)
    start_r = np.full(B, bit[25] | (bit[24] << 1) | (bit[23] << 2) | (bit[22] << 3))
    start_l = np.full(B, bit[0] | (bit[1] << 1) | (bit[2] << 2) | (bit[3] << 3))
    with np.errstate(all="ignore"):
        Dr = _half(yr, yi, w, hr, hi, start_r, False)
        Dl = _half(yr, yi, w, hr[:, :, ::-1], hi[:, :, ::-1], start_l, True)
        den = (F(8.0) * E.astype(F))[:, None]
        sr = F(0.5) + Dr / den
        sl = F(0.5) + Dl / den
        sr = np.where(sr > F(1.0), F(1.0), sr); sr = np.where(sr < F(0.0), F(0.0), sr)
        sl = np.where(sl > F(1.0), F(1.0), sl); sl = np.where(sl < F(0.0), F(0.0), sl)
    soft = slicer(yr[np.arange(B), primary])
    soft[:, 87:148] = sr
    soft[:, 60::-1] = sl                                      # step i is symbol 60 - i
    return soft.astype(F)


def equalise(y, tsc, primary=None):
    """Steps 2-5 on symbols y [B, 2, 148]: (soft [B, 148] float32, win [B] int32 (w, or 1 = fell back), h [B, 2, 5] complex64 (zeros
    on fallback))."""
    y = np.ascontiguousarray(y, np.complex64)
    B = y.shape[0]
    primary = np.zeros(B, np.int64) if primary is None else np.asarray(primary, np.int64)
    t = tsc_symbols(tsc)
    with np.errstate(all="ignore"):
        fine = (np.abs(y.real) < F(2.0 ** 30)).all(axis=(1, 2)) & (np.abs(y.imag) < F(2.0 ** 30)).all(axis=(1, 2))   # either antenna's
        ys = np.where(fine[:, None, None], y, 0).astype(np.complex64)     # (a burst that falls back runs through below on zeros, unused)
        _, w, h, E = estimate(ys, t)
        ok = fine & (E != 0)
        eq = trellis(ys, tsc, w, h, E, primary)
    yp = y[np.arange(B), primary]
    soft = np.where(ok[:, None], eq, slicer(yp.real.astype(F))).astype(F)
    win = np.where(ok, w, WIN_FELL_BACK).astype(np.int32)
    h = np.where(ok[:, None, None], h, 0).astype(np.complex64)
    return soft, win, h


def mlse_div_batch(sps, x0, off0, x1, off1, length, tsc, amp, toa, primary=None, enable=None, nsoft=148, oracle=None):
    """trxsig_mlse_div_batch on packed bursts: dict(soft [B, nsoft], hard, win [B], chan [B, 2, 5], y [B, 2, 148])."""
    o = oracle or oraclebind.Oracle(sps)
    B = len(off0)
    amp = np.broadcast_to(np.asarray(amp, np.complex64), (B,)); toa = np.broadcast_to(np.asarray(toa, np.float32), (B,))
    primary = np.zeros(B, np.int64) if primary is None else (np.asarray(primary) != 0).astype(np.int64)
    y = np.zeros((B, 2, 148), np.complex64)
    state = np.zeros(B, np.int32)
    for b in range(B):
        # the geometry test once for the burst: the antennas share length and TOA, both offsets have to pass
        if (enable is not None and not enable[b]) or not burst_enabled(sps, int(off0[b]), int(length[b]), toa[b]) or int(off1[b]) < 0:
            state[b] = WIN_SKIPPED
            continue
        y[b, 0] = symbols(o, x0[off0[b]:off0[b] + length[b]], amp[b], toa[b])
        y[b, 1] = symbols(o, x1[off1[b]:off1[b] + length[b]], amp[b], toa[b])
        if length[b] // sps < 148:
            state[b] = WIN_FELL_BACK
    soft, win, h = equalise(y, tsc, primary)
    short = state == WIN_FELL_BACK
    if short.any():
        soft[short] = slicer(y[short, primary[short]].real)
        win[short] = WIN_FELL_BACK; h[short] = 0
    skip = state == WIN_SKIPPED
    soft[skip] = 0; win[skip] = WIN_SKIPPED; h[skip] = 0
    soft = np.ascontiguousarray(soft[:, :nsoft])
    with np.errstate(all="ignore"):
        hard = (soft > F(0.5)).astype(np.uint8)
    return dict(soft=soft, hard=hard, win=win, chan=h, y=y)


def select(valid0, amp0, valid1, amp1):
    """The selection rule of trxsig_mlse_div_normal_batch / trxsig_trxgroup_combine_div: sel [B] uint8.  n_a = re*re + im*im in
    float32; sel = 1 if v_1 && (!v_0 || n_1 > n_0) (a NaN compares false); else 0 if v_0; else 2."""
    v0 = np.asarray(valid0) != 0; v1 = np.asarray(valid1) != 0
    a0 = np.asarray(amp0, np.complex64); a1 = np.asarray(amp1, np.complex64)
    with np.errstate(all="ignore"):
        n0 = a0.real.astype(F) * a0.real.astype(F) + a0.imag.astype(F) * a0.imag.astype(F)
        n1 = a1.real.astype(F) * a1.real.astype(F) + a1.imag.astype(F) * a1.imag.astype(F)
        one = v1 & (~v0 | (n1 > n0))
    return np.where(one, 1, np.where(v0, 0, 2)).astype(np.uint8)
