"""The float32 model of the two-antenna sequence equaliser with interference-rejection combining (trxsig_mlse_irc_batch,
csrc/trxsig_mlse_irc.hip): the algorithm of include/trxsig.h restated in numpy float32, operation by operation, vectorised over
bursts.  The kernel must equal it word for word.  It is tests/mlse_div_model.py with steps 2b-2d added and det in the branch
metric: the estimator and the selection are that module's, by import, the expected values, the trellis and the batch wrapper
tests/mlse_core.py's; the residual sums, the set, the whitening and the branch metric are stated here.

Every arithmetic step below is ONE float32 operation on float32 arrays, in the order the header states."""
import numpy as np

import mlse_core as core
from mlse_core import F, INF, WIN_FELL_BACK, WIN_SKIPPED  # noqa: F401  (the importers' names)
from mlse_div_model import estimate, select  # noqa: F401  (select: the callers' rule)
from mlse_model import LEFT0, RIGHT0, STEPS, slicer, start_states, tsc_symbols

LOADING = F(1.0 / 64.0)                                       # what the tools and the Transceiver groups use
IDENTITY = np.array([1.0, 1.0, 0.0, 0.0], F)


def residual_sums(y, w, h, t):
    """Step 2b on symbols y [B, 2, 148], windows w [B], taps h [B, 2, 5], training symbols t [26]: (S00, S11, Xr, Xi), each [B]."""
    B = y.shape[0]
    rows = np.arange(B)
    yr, yi = y.real.astype(F), y.imag.astype(F)
    Z0r, Z0i = core.expected(h[:, 0].real.astype(F), h[:, 0].imag.astype(F))
    Z1r, Z1i = core.expected(h[:, 1].real.astype(F), h[:, 1].imag.astype(F))
    bit = (t > 0).astype(np.int64)
    S00 = np.zeros(B, F); S11 = np.zeros(B, F); Xr = np.zeros(B, F); Xi = np.zeros(B, F)
    for m in range(65, 87):
        x = sum(int(bit[m - 61 - k]) << k for k in range(5))   # bit k of x_m = training bit m - 61 - k
        n = m + w
        r0r = yr[rows, 0, n] - Z0r[:, x]; r0i = yi[rows, 0, n] - Z0i[:, x]
        r1r = yr[rows, 1, n] - Z1r[:, x]; r1i = yi[rows, 1, n] - Z1i[:, x]
        S00 = S00 + (r0r * r0r + r0i * r0i)
        S11 = S11 + (r1r * r1r + r1i * r1i)
        Xr = Xr + (r0r * r1r + r0i * r1i)
        Xi = Xi + (r0i * r1r - r0r * r1i)
    return S00, S11, Xr, Xi


def covariance_set(S00, S11, Xr, Xi, loading, cov_in=None):
    """Step 2c: (A, Bv, xr, xi, det), each [B] float32, the identity set (1, 1, 0, 0; det 1) where the set cannot be used."""
    if cov_in is None:
        tt = S00 + S11
        ident = ~(tt > F(0.0))
        A = S00 / tt + F(loading); Bv = S11 / tt + F(loading); xr = Xr / tt; xi = Xi / tt
    else:
        cov_in = np.asarray(cov_in, F)
        A, Bv, xr, xi = (cov_in[:, k].copy() for k in range(4))
        ident = np.zeros(len(A), bool)
    det = A * Bv - (xr * xr + xi * xi)
    lim = F(2.0 ** 10)
    ident = ident | ~(A < lim) | ~(Bv < lim) | ~(np.abs(xr) < lim) | ~(np.abs(xi) < lim) | ~(A >= F(0.0)) | ~(Bv >= F(0.0)) | ~(det > F(0.0))
    one, zero = F(1.0), F(0.0)
    return (np.where(ident, one, A).astype(F), np.where(ident, one, Bv).astype(F), np.where(ident, zero, xr).astype(F),
            np.where(ident, zero, xi).astype(F), np.where(ident, one, det).astype(F))


def whiten(A, xr, xi, v0r, v0i, v1r, v1i):
    """Step 2d's map on float32 arrays (A, xr, xi broadcast against the values): (re, im) of A v1 - conj(x) v0."""
    wr = A * v1r - (xr * v0r + xi * v0i)
    wi = A * v1i - (xr * v0i - xi * v0r)
    return wr, wi


def metric(yr, yi, gr, gi, det):
    """The branch metrics as core.half takes them: mlse_div_model.metric with det [B] on antenna 0's term.  yr, yi [B, 2, 148]
    (antenna 1 whitened); gr, gi [B, 2, 5] (antenna 1's whitened)."""
    Z0r, Z0i = core.expected(gr[:, 0], gi[:, 0])
    Z1r, Z1i = core.expected(gr[:, 1], gi[:, 1])
    rows = np.arange(yr.shape[0])

    def at(n):
        dr0 = yr[rows, 0, n][:, None] - Z0r; di0 = yi[rows, 0, n][:, None] - Z0i
        dr1 = yr[rows, 1, n][:, None] - Z1r; di1 = yi[rows, 1, n][:, None] - Z1i
        g = det[:, None] * (dr0 * dr0 + di0 * di0) + (dr1 * dr1 + di1 * di1)
        return g
    return at


def trellis(y, tsc, w, h0, h1w, cov, det, E, Ew, primary=None):
    """Steps 2d (the symbols' whitening), 3 and 4 on UNWHITENED symbols y [B, 2, 148] with windows w, antenna 0's taps h0 [B, 5], antenna
    1's whitened taps h1w [B, 5], the set cov [B, 4], det, E and E_w [B]: soft [B, 148] float32 (the demodulator's formula on the
    unwhitened primary antenna on 61..86)."""
    y = np.ascontiguousarray(y, np.complex64)
    B = y.shape[0]
    primary = np.zeros(B, np.int64) if primary is None else np.asarray(primary, np.int64)
    yr, yi = y.real.astype(F), y.imag.astype(F)
    A, xr, xi = cov[:, 0], cov[:, 2], cov[:, 3]
    start_r, start_l = start_states(tsc_symbols(tsc), B)
    with np.errstate(all="ignore"):
        y1r, y1i = whiten(A[:, None], xr[:, None], xi[:, None], yr[:, 0], yi[:, 0], yr[:, 1], yi[:, 1])
        ywr = np.stack([yr[:, 0], y1r], axis=1); ywi = np.stack([yi[:, 0], y1i], axis=1)
        hr = np.stack([h0.real.astype(F), h1w.real.astype(F)], axis=1); hi = np.stack([h0.imag.astype(F), h1w.imag.astype(F)], axis=1)
        Dr = core.half(metric(ywr, ywi, hr, hi, det), w, start_r, STEPS, RIGHT0, False)
        Dl = core.half(metric(ywr, ywi, hr[:, :, ::-1], hi[:, :, ::-1], det), w, start_l, STEPS, LEFT0, True)
        den_E = Ew.astype(F)
        den = (F(8.0) * den_E)[:, None]
        sr = core.soft_out(Dr, den)
        sl = core.soft_out(Dl, den)
    soft = slicer(yr[np.arange(B), primary])
    soft[:, RIGHT0:148] = sr
    soft[:, LEFT0::-1] = sl                                   # step i is symbol 60 - i
    return soft.astype(F)


def equalise(y, tsc, primary=None, loading=LOADING, cov_in=None):
    """Steps 2-5 on symbols y [B, 2, 148]: dict(soft [B, 148] float32; win [B] int32 (w, or 1 = fell back); chan [B, 2, 5] complex64,
    the unwhitened taps (zeros on fallback); cov [B, 4] float32, the set used (zeros on fallback); and for the grading: sums [B, 4]
    (S00, S11, Xr, Xi), det [B], Ew [B], h1w [B, 5])."""
    y = np.ascontiguousarray(y, np.complex64)
    B = y.shape[0]
    primary = np.zeros(B, np.int64) if primary is None else np.asarray(primary, np.int64)
    t = tsc_symbols(tsc)
    fine, ys = core.usable(y)                                 # either antenna's
    with np.errstate(all="ignore"):
        _, w, h, E = estimate(ys, t)
        ok = fine & (E != 0)
        S00, S11, Xr, Xi = residual_sums(ys, w, h, t)
        A, Bv, xr, xi, det = covariance_set(S00, S11, Xr, Xi, loading, cov_in)
        h0r, h0i = h[:, 0].real.astype(F), h[:, 0].imag.astype(F)
        h1r, h1i = h[:, 1].real.astype(F), h[:, 1].imag.astype(F)
        wr, wi = whiten(A[:, None], xr[:, None], xi[:, None], h0r, h0i, h1r, h1i)
        pw = det[:, None] * (h0r * h0r + h0i * h0i) + (wr * wr + wi * wi)
        Ew = (((pw[:, 0] + pw[:, 1]) + pw[:, 2]) + pw[:, 3]) + pw[:, 4]
        back = ~(Ew > F(0.0)) | ~np.isfinite(Ew)               # the identity set after all, and then E_w is E
        one, zero = F(1.0), F(0.0)
        A = np.where(back, one, A).astype(F); Bv = np.where(back, one, Bv).astype(F)
        xr = np.where(back, zero, xr).astype(F); xi = np.where(back, zero, xi).astype(F); det = np.where(back, one, det).astype(F)
        Ew = np.where(back, E, Ew).astype(F)
        wr, wi = whiten(A[:, None], xr[:, None], xi[:, None], h0r, h0i, h1r, h1i)
        h1w = (wr + 1j * wi).astype(np.complex64)
        cov = np.stack([A, Bv, xr, xi], axis=1).astype(F)
        eq = trellis(ys, tsc, w, h[:, 0], h1w, cov, det, E, Ew, primary)
    soft, win, h = core.fall_back(ok, eq, y[np.arange(B), primary], w, h)
    cov = np.where(ok[:, None], cov, 0).astype(F)
    return dict(soft=soft, win=win, chan=h, cov=cov, sums=np.stack([S00, S11, Xr, Xi], axis=1), det=det, Ew=Ew, h1w=h1w)


def mlse_irc_batch(sps, x0, off0, x1, off1, length, tsc, amp, toa, primary=None, enable=None, loading=LOADING, cov_in=None, nsoft=148,
                   oracle=None, y=None):
    """trxsig_mlse_irc_batch on packed bursts: dict(soft [B, nsoft], hard, win [B], chan [B, 2, 5], cov [B, 4], y [B, 2, 148], ...).
    y: the symbols of an earlier run of this or of mlse_div_model.mlse_div_batch on the same bursts, amp and TOA (step 1 is the same;
    it is the slow part), or None."""
    return core.batch(lambda y, primary: equalise(y, tsc, primary, loading, cov_in), sps, [x0, x1], [off0, off1], length, amp, toa,
                      primary=primary, enable=enable, nsoft=nsoft, oracle=oracle, y=y, zeroed=("chan", "cov"))


