"""The float64 reference of the fit detector's statistic (trxsig_sch_fit_batch, steps 3 to 5): the residual of the five-tap fit on
the rows 46..101, R and q in float64 from the float32 symbols, window and taps, written as plain matrix arithmetic; and the a-priori
bound on what float32 may make of them.  tests/sch_fit_model.py and the kernel are graded against it (tests/test_sch_fit_model.py,
tests/test_gpu_sch_fit.py).  Nothing is shared with the model or the kernel.

The operation.  a[42 + i] = 2 XTS[i] - 1;  r[n] = y[n] - sum_{k=0..4} h[k] a[n - w - k], n = 46..101;  e[n] = |r[n]|^2;
R = sum e[n];  E = sum_k |h[k]|^2;  q = sqrt(51 E / R).

The bound, from the roundings alone (u = 2^-24; g_k = k u / (1 - k u) bounds the relative error of k roundings in a row):
  * Z[n], per component: h[0] a is exact (a sign flip), then four rounded additions: every term is carried through at most four
    roundings, |Z32 - Z| <= g_4 H, H = sum_k |h[k]| of that component.
  * r32 = fl(y - Z32) = (r + (Z - Z32)) (1 + eps), |eps| <= u:   |r32 - r| <= d = u |r| + (1 + u) g_4 H   per component.
  * e32 = fl(fl(r32.re^2) + fl(r32.im^2)) = (r32.re^2 + r32.im^2) (1 + t), |t| <= g_2, and |r32^2 - r^2| <= 2 |r| d + d^2:
        |e32 - e| <= b = (1 + g_2) (2 (|r.re| d.re + |r.im| d.im) + d.re^2 + d.im^2) + g_2 e.
  * R32: 55 additions of non-negative numbers in a tree six levels deep (the eight zeros add exactly): every e32 is carried
    through at most six roundings:  |R32 - R| <= bR = sum b + g_6 (R + sum b).
  * E32 = E (1 + t), |t| <= g_6 (tests/mlse_sch_ref.py: two-rounding products, four additions); 51 E32 rounds once, the quotient
    once: the radicand is 51 E / R times (1 + t') / (1 + rho), |t'| <= g_8, |rho| <= bR / R; the root rounds once:
        |q32 - q| <= bq = q (sqrt((1 + g_8) / (1 - bR / R)) (1 + u) - 1)        (needs bR < R; the lower side is smaller).
The 1.001 of tests/mlse_ref.py (SLACK) covers the float64 arithmetic of this file.  Nothing here was fitted to an observed error.
"""
import numpy as np

from fectxbind import XTS_BITS
from mlse_ref import SLACK, U

ROWS = np.arange(46, 102)
NDOF = 51.0
XTS = np.array([int(v) for v in XTS_BITS], np.int64)


def _g(k):
    return k * U / (1.0 - k * U)


def fit64(y, w, h):
    """The reference on symbols y [B, 148] (complex64), windows w [B] and taps h [B, 5] (complex64): dict(R, q, E [B] float64,
    bound_R, bound_q [B] (bound_q inf where bR >= R), r [B, 56] complex)."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    h = np.ascontiguousarray(h, np.complex64).astype(np.complex128)
    w = np.asarray(w, np.int64)
    assert y.ndim == 2 and y.shape[1] == 148 and h.shape == (y.shape[0], 5) and np.all((w >= -4) & (w <= 0))
    a = np.zeros(148); a[42:106] = 2.0 * XTS - 1.0
    idx = ROWS[None, :, None] - w[:, None, None] - np.arange(5)[None, None, :]         # [B, 56, 5]
    assert idx.min() >= 42 and idx.max() <= 105
    Z = (a[idx] * h[:, None, :]).sum(axis=2)
    r = y[:, ROWS] - Z
    e = r.real ** 2 + r.imag ** 2
    R = e.sum(axis=1)
    E = (h.real ** 2 + h.imag ** 2).sum(axis=1)
    Hr, Hi = np.abs(h.real).sum(axis=1)[:, None], np.abs(h.imag).sum(axis=1)[:, None]
    dr = U * np.abs(r.real) + (1.0 + U) * _g(4) * Hr
    di = U * np.abs(r.imag) + (1.0 + U) * _g(4) * Hi
    b = (1.0 + _g(2)) * (2.0 * (np.abs(r.real) * dr + np.abs(r.imag) * di) + dr ** 2 + di ** 2) + _g(2) * e
    sb = b.sum(axis=1)
    bR = SLACK * (sb + _g(6) * (R + sb))
    with np.errstate(all="ignore"):
        q = np.sqrt(NDOF * E / R)
        rho = bR / R
        bq = np.where(rho < 1.0, SLACK * q * (np.sqrt((1.0 + _g(8)) / np.where(rho < 1.0, 1.0 - rho, 1.0)) * (1.0 + U) - 1.0), np.inf)
    return dict(R=R, q=q, E=E, bound_R=bR, bound_q=bq, r=r)


def grade(R32, q32, y, w, h):
    """dict(ratio_R, ratio_q [B]: error / bound; ok_R, ok_q [B]; ref)."""
    ref = fit64(y, w, h)
    with np.errstate(all="ignore"):
        eR = np.abs(np.asarray(R32, np.float64) - ref["R"]); eq = np.abs(np.asarray(q32, np.float64) - ref["q"])
        ratio_R = eR / ref["bound_R"]; ratio_q = eq / ref["bound_q"]
    return dict(ratio_R=ratio_R, ratio_q=ratio_q, ok_R=eR <= ref["bound_R"], ok_q=eq <= ref["bound_q"], ref=ref)
