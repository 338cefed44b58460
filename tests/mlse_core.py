"""What the float32 models of the sequence equalisers share (tests/mlse_model.py, mlse_div_model.py, mlse_irc_model.py,
mlse_access_model.py, mlse_sch_model.py, sch_fit_model.py): the symbols of a burst and the demodulator's slicer, the expected
values, the window choice, the one 16-state trellis, the soft-bit formula, the least-squares tap loop, the guards of step 2 and the
batch wrapper.  Each stands here once, as csrc/trxsig_mlse_dev.h holds the kernels' shared device code once; a model file keeps
its estimator rule, its branch metric, its start states and its step-to-symbol map.

Every arithmetic step below is ONE float32 operation on float32 arrays (numpy rounds each separately; nothing here is a float64
intermediate), in the order include/trxsig.h states.  The symbols come from the CPU oracle's scale_vector / delay_vector /
gmsk_rotate with the reference's 1/amp (cinv, then the product with (1, 0)).
"""
import numpy as np

import oraclebind

F = np.float32
INF = F(np.inf)
WIN_FELL_BACK, WIN_SKIPPED = 1, 2


# ---- step 1: a burst's symbols -------------------------------------------------------------------------------------------------------
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


# ---- step 2: the estimate ------------------------------------------------------------------------------------------------------------
def ls_estimate(y, P, row0):
    """The pseudo-inverse tap loop on symbols y [B, 148] with the float32 table P [9, rows]: c[k] = sum_j P[k][j] y[row0 + j], j
    ascending from 0, as (re, im) [B, 9] float32."""
    B = y.shape[0]
    ntap, nrow = P.shape
    yr, yi = y.real.astype(F), y.imag.astype(F)
    cr = np.zeros((B, ntap), F); ci = np.zeros((B, ntap), F)
    for k in range(ntap):
        ar = np.zeros(B, F); ai = np.zeros(B, F)
        for j in range(nrow):
            ar = ar + P[k, j] * yr[:, row0 + j]
            ai = ai + P[k, j] * yi[:, row0 + j]
        cr[:, k] = ar; ci[:, k] = ai
    return cr, ci


def window(p):
    """The window of the nine tap powers p [B, 9] (d = -4..4): (w [B] int32 in -4..0, E [B] float32)."""
    B = p.shape[0]

    def energy(w):
        k = w + 4
        return (((p[:, k] + p[:, k + 1]) + p[:, k + 2]) + p[:, k + 3]) + p[:, k + 4]
    E = energy(0); w = np.zeros(B, np.int32)
    for q in range(1, 5):
        Ew = energy(-q)
        take = Ew > E                                          # a later window only on a strict >
        E = np.where(take, Ew, E); w = np.where(take, -q, w).astype(np.int32)
    return w, E.astype(F)


def taps(c, w):
    """h[k] = c[w + k], k = 0..4, of one antenna's nine taps c [B, 9] (complex64): [B, 5]."""
    idx = (w + 4)[:, None] + np.arange(5)[None, :]
    return c[np.arange(c.shape[0])[:, None], idx]


def usable(y):
    """The guard of step 2 on symbols y [B, 148] or [B, 2, 148]: (fine [B]: every component of every antenna below 2^30 in
    magnitude; ys: y with the other bursts zeroed -- a burst that falls back runs through the steps on zeros, unused)."""
    axes = tuple(range(1, y.ndim))
    with np.errstate(all="ignore"):
        fine = (np.abs(y.real) < F(2.0 ** 30)).all(axis=axes) & (np.abs(y.imag) < F(2.0 ** 30)).all(axis=axes)
    return fine, np.where(fine.reshape((-1,) + (1,) * len(axes)), y, 0).astype(np.complex64)


def fall_back(ok, eq, yp, w, h):
    """Step 5: (soft [B, 148], win [B] int32, h) -- the equalised row eq, the window and the taps where ok; the slicer on the
    (primary antenna's) symbols yp [B, 148], the word WIN_FELL_BACK and zero taps elsewhere."""
    soft = np.where(ok[:, None], eq, slicer(yp.real.astype(F))).astype(F)
    win = np.where(ok, w, WIN_FELL_BACK).astype(np.int32)
    return soft, win, np.where(ok.reshape((-1,) + (1,) * (h.ndim - 1)), h, 0).astype(np.complex64)


# ---- steps 3 and 4: the trellis -----------------------------------------------------------------------------------------------------
def expected(gr, gi):
    """Z[x], x = 0..31, of taps g [B, 5]: (re, im) [B, 32]; starts from +-g[0], adds k = 1..4 in order."""
    x = np.arange(32)
    sign = np.where(((x[:, None] >> np.arange(5)[None, :]) & 1) == 1, F(1.0), F(-1.0)).astype(F)     # [32, 5]
    Zr = gr[:, None, 0] * sign[None, :, 0]; Zi = gi[:, None, 0] * sign[None, :, 0]
    for k in range(1, 5):
        Zr = Zr + gr[:, None, k] * sign[None, :, k]
        Zi = Zi + gi[:, None, k] * sign[None, :, k]
    return Zr, Zi


def half(metric, w, start, steps, first, left, force_tail=True, sign_w=1):
    """The one trellis, for every burst at once: M_0 - M_1 per step, [B, steps].  metric(n) gives the 32 branch metrics [B, 32]
    float32 of the step that reads sample n [B] (entry x: the step's symbol is bit 0 of x, the four before it bits 1..4); w [B] the
    windows; start (a word, or [B]) the state the known symbols before the first step leave.  Step i is symbol first + i on sample
    first + i + w, or, walking left, symbol first - i on sample first - i + 4 + w; the last three steps are tail symbols (force_tail).
    sign_w = -1: the mutant of tests/test_mlse_access_model.py."""
    B = len(w)
    gam = np.zeros((steps, B, 32), F)
    for i in range(steps):
        g = metric((first - i + 4 + sign_w * w) if left else (first + i + sign_w * w))
        if force_tail and i >= steps - 3:
            g[:, 1::2] = INF                                   # the tail symbols are -1: b = 1 contradicts
        gam[i] = g
    s = np.arange(16)
    alpha = np.where(s[None, :] == np.broadcast_to(start, (B,))[:, None], F(0.0), INF).astype(F)
    A = np.zeros((steps, B, 16), F)
    p0, p1 = s >> 1, (s >> 1) | 8
    for i in range(steps):
        alpha = np.minimum(alpha[:, p0] + gam[i][:, s], alpha[:, p1] + gam[i][:, s | 16])     # x = (pred << 1) | b
        A[i] = alpha
    beta = np.zeros((B, 16), F)
    D = np.zeros((B, steps), F)
    for i in range(steps - 1, -1, -1):
        T = A[i] + beta
        D[:, i] = T[:, 0::2].min(axis=1) - T[:, 1::2].min(axis=1)
        x0, x1 = 2 * s, 2 * s + 1
        beta = np.minimum(gam[i][:, x0] + beta[:, x0 & 15], gam[i][:, x1] + beta[:, x1 & 15])
    return D


def soft_out(D, den):
    """0.5 + D / den, clamped to [0, 1] with the demodulator's comparisons (a NaN stays a NaN).  den: 8 E, [B, 1]."""
    s = F(0.5) + D / den
    s = np.where(s > F(1.0), F(1.0), s)
    return np.where(s < F(0.0), F(0.0), s)


# ---- the batch entry points -----------------------------------------------------------------------------------------------------------
def burst_symbols(sps, xs, offs, length, amp, toa, enable=None, oracle=None, y=None):
    """The symbols of packed bursts, one (x, off) per antenna: (y [B, antennas, 148] complex64, zeros for a skipped burst; state [B]:
    0, WIN_FELL_BACK for a short burst, WIN_SKIPPED for one that is disabled or fails the geometry test -- once for the burst: the
    antennas share length and TOA, every offset has to pass).  y: the symbols of an earlier run on the same bursts, amp and TOA."""
    B = len(offs[0])
    amp = np.broadcast_to(np.asarray(amp, np.complex64), (B,)); toa = np.broadcast_to(np.asarray(toa, np.float32), (B,))
    have = y is not None
    y = np.array(y, np.complex64).reshape(B, len(xs), 148) if have else np.zeros((B, len(xs), 148), np.complex64)
    o = None if have else (oracle or oraclebind.Oracle(sps))
    state = np.zeros(B, np.int32)
    for b in range(B):
        if (enable is not None and not enable[b]) or not burst_enabled(sps, int(offs[0][b]), int(length[b]), toa[b]) \
                or any(int(off[b]) < 0 for off in offs[1:]):
            state[b] = WIN_SKIPPED
            y[b] = 0
            continue
        if not have:
            for a, (x, off) in enumerate(zip(xs, offs)):
                y[b, a] = symbols(o, x[off[b]:off[b] + length[b]], amp[b], toa[b])
        if length[b] // sps < 148:
            state[b] = WIN_FELL_BACK
    return y, state


def batch(equalise, sps, xs, offs, length, amp, toa, primary=None, enable=None, nsoft=148, oracle=None, y=None, zeroed=("chan",)):
    """A trxsig_mlse_*_batch call on packed bursts, one (x, off) per antenna: dict(soft [B, nsoft], hard, win [B], y, and what
    equalise(y, primary) gives besides -- (soft, win, chan), or a dict with these).  A short burst gets the slicer on its primary
    antenna and the word WIN_FELL_BACK, a skipped one zeros and WIN_SKIPPED; both get zeros in the outputs named by `zeroed`."""
    B = len(offs[0])
    primary = np.zeros(B, np.int64) if primary is None else (np.asarray(primary) != 0).astype(np.int64)
    y, state = burst_symbols(sps, xs, offs, length, amp, toa, enable, oracle, y)
    ys = y if len(xs) > 1 else y[:, 0]
    r = equalise(ys, primary)
    r = dict(r) if isinstance(r, dict) else dict(zip(("soft", "win", "chan"), r))
    soft, win = r["soft"], r["win"]
    short = state == WIN_FELL_BACK
    if short.any():
        soft[short] = slicer(y[short, primary[short]].real)
    soft[state == WIN_SKIPPED] = 0
    out_ = state != 0
    win[out_] = state[out_]
    for k in zeroed:
        r[k][out_] = 0
    r["soft"] = np.ascontiguousarray(soft[:, :nsoft])
    with np.errstate(all="ignore"):
        r["hard"] = (r["soft"] > F(0.5)).astype(np.uint8)
    r["y"] = ys
    return r
