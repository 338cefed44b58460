"""The float32 model of the sequence equaliser for access bursts (trxsig_mlse_access_batch, csrc/trxsig_mlse_access.hip): the
algorithm of include/trxsig.h restated in numpy float32, operation by operation, vectorised over bursts.  The kernel must equal
it word for word.

Every arithmetic step below is ONE float32 operation on float32 arrays, in the order the header states.  The symbols are
tests/mlse_model.py's (the CPU oracle's scale_vector / delay_vector / gmsk_rotate); the least-squares table is derived here
from Python integers and must equal the committed one (csrc/trxsig_mlse_access_tab.h) word for word.
"""
import functools
from fractions import Fraction

import numpy as np

import l1_ms_model as lms
import mlse_model
import oraclebind

F = np.float32
INF = F(np.inf)
WIN_FELL_BACK, WIN_SKIPPED = mlse_model.WIN_FELL_BACK, mlse_model.WIN_SKIPPED
NTAP, NROW = 9, 41                                            # c[-4..4]; the positions n = 4..44 whose nine symbols are all known
FIRST, STEPS = 49, 39                                         # the trellis decides symbols 49..87: 36 coded bits and 3 tail bits
HEAD = (2 * lms.ACCESS_HEAD.astype(np.int64) - 1)             # a[0..48]
START = int(lms.ACCESS_HEAD[48]) | int(lms.ACCESS_HEAD[47]) << 1 | int(lms.ACCESS_HEAD[46]) << 2 | int(lms.ACCESS_HEAD[45]) << 3


def design_matrix():
    """A [41][9] of Python integers: A[n - 4][d + 4] = a[n - d], n = 4..44, d = -4..4."""
    return [[int(HEAD[n - d]) for d in range(-4, 5)] for n in range(4, 45)]


def _det_adj(G):
    """(det, adj) of a square matrix of Python integers, exactly: Gauss-Jordan on Fractions, adj = det * inverse."""
    n = len(G)
    M = [[Fraction(v) for v in row] + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(G)]
    det = Fraction(1)
    for col in range(n):
        piv = next(r for r in range(col, n) if M[r][col] != 0)
        if piv != col:
            M[col], M[piv] = M[piv], M[col]
            det = -det
        det *= M[col][col]
        inv = 1 / M[col][col]
        M[col] = [v * inv for v in M[col]]
        for r in range(n):
            if r != col and M[r][col] != 0:
                f = M[r][col]
                M[r] = [a - f * b for a, b in zip(M[r], M[col])]
    assert det.denominator == 1
    adj = [[M[i][n + j] * det for j in range(n)] for i in range(n)]
    assert all(v.denominator == 1 for row in adj for v in row)
    return int(det), [[int(v) for v in row] for row in adj]


@functools.lru_cache(maxsize=None)
def pinv_integers():
    """(N [9][41], det): N = adj(A^T A) A^T and det(A^T A), Python integers; the least-squares estimator is N / det."""
    A = design_matrix()
    G = [[sum(A[n][i] * A[n][j] for n in range(NROW)) for j in range(NTAP)] for i in range(NTAP)]
    det, adj = _det_adj(G)
    N = [[sum(adj[i][k] * A[n][k] for k in range(NTAP)) for n in range(NROW)] for i in range(NTAP)]
    return N, det


@functools.lru_cache(maxsize=None)
def pinv_table():
    """P32 [9, 41] float32: (float)((double)N / (double)det), one correctly rounded double division of two exactly representable
    integers (Python's int / int is correctly rounded too, and the same here: both are below 2^53), then one rounding to float32."""
    N, det = pinv_integers()
    assert abs(det) < 2 ** 53 and all(abs(v) < 2 ** 53 for row in N for v in row)
    P = np.array([[float(v) / float(det) for v in row] for row in N], np.float64).astype(F)
    P.setflags(write=False)
    return P


def estimate(y, P32=None):
    """Step 2 on symbols y [B, 148] (complex64): (c [B, 9] for d = -4..4, w [B], h [B, 5], E [B])."""
    P = pinv_table() if P32 is None else np.asarray(P32, F)
    B = y.shape[0]
    yr, yi = y.real.astype(F), y.imag.astype(F)
    cr = np.zeros((B, NTAP), F); ci = np.zeros((B, NTAP), F)
    for k in range(NTAP):
        ar = np.zeros(B, F); ai = np.zeros(B, F)
        for j in range(NROW):
            ar = ar + P[k, j] * yr[:, 4 + j]
            ai = ai + P[k, j] * yi[:, 4 + j]
        cr[:, k] = ar; ci[:, k] = ai
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


def _run(yr, yi, w, gr, gi, start, force_tail=True, sign_w=1):
    """The one trellis of every burst: M_0 - M_1 per step, [B, 39].  yr, yi [B, 148]; gr, gi [B, 5]."""
    B = yr.shape[0]
    x = np.arange(32)
    sign = np.where(((x[:, None] >> np.arange(5)[None, :]) & 1) == 1, F(1.0), F(-1.0)).astype(F)     # [32, 5]
    Zr = gr[:, None, 0] * sign[None, :, 0]; Zi = gi[:, None, 0] * sign[None, :, 0]
    for k in range(1, 5):
        Zr = Zr + gr[:, None, k] * sign[None, :, k]
        Zi = Zi + gi[:, None, k] * sign[None, :, k]
    rows = np.arange(B)
    gam = np.zeros((STEPS, B, 32), F)
    for i in range(STEPS):
        n = FIRST + i + sign_w * w
        dr = yr[rows, n][:, None] - Zr; di = yi[rows, n][:, None] - Zi
        g = dr * dr + di * di
        if i >= 36 and force_tail:
            g[:, 1::2] = INF                                   # the tail symbols are -1: b = 1 contradicts
        gam[i] = g
    s = np.arange(16)
    alpha = np.where(s[None, :] == start, F(0.0), INF).astype(F) * np.ones((B, 1), F)
    A = np.zeros((STEPS, B, 16), F)
    p0, p1 = s >> 1, (s >> 1) | 8
    for i in range(STEPS):
        alpha = np.minimum(alpha[:, p0] + gam[i][:, s], alpha[:, p1] + gam[i][:, s | 16])     # x = (pred << 1) | b
        A[i] = alpha
    beta = np.zeros((B, 16), F)
    D = np.zeros((B, STEPS), F)
    for i in range(STEPS - 1, -1, -1):
        T = A[i] + beta
        D[:, i] = T[:, 0::2].min(axis=1) - T[:, 1::2].min(axis=1)
        x0, x1 = 2 * s, 2 * s + 1
        beta = np.minimum(gam[i][:, x0] + beta[:, x0 & 15], gam[i][:, x1] + beta[:, x1 & 15])
    return D


def trellis(y, w, h, E, start=START, force_tail=True, sign_w=1):
    """Steps 3-4 on symbols y [B, 148] with given windows, taps and energies: soft [B, 148] float32 (the demodulator's formula
    on 0..48 and 88..147).  start / force_tail / sign_w: the mutants of tests/test_mlse_access_model.py."""
    y = np.ascontiguousarray(y, np.complex64)
    yr, yi = y.real.astype(F), y.imag.astype(F)
    with np.errstate(all="ignore"):
        D = _run(yr, yi, w, h.real.astype(F), h.imag.astype(F), start, force_tail, sign_w)
        den = (F(8.0) * E.astype(F))[:, None]
        s = F(0.5) + D / den
        s = np.where(s > F(1.0), F(1.0), s); s = np.where(s < F(0.0), F(0.0), s)
    soft = mlse_model.slicer(yr)
    soft[:, FIRST:FIRST + STEPS] = s
    return soft.astype(F)


def equalise(y, **mutant):
    """Steps 2-5 on symbols y [B, 148]: (soft [B, 148] float32, win [B] int32 (w, or 1 = fell back), h [B, 5] complex64)."""
    y = np.ascontiguousarray(y, np.complex64)
    P32 = mutant.pop("P32", None)
    with np.errstate(all="ignore"):
        fine = (np.abs(y.real) < F(2.0 ** 30)).all(axis=1) & (np.abs(y.imag) < F(2.0 ** 30)).all(axis=1)
        ys = np.where(fine[:, None], y, 0).astype(np.complex64)     # (a burst that falls back runs through below on zeros, unused)
        _, w, h, E = estimate(ys, P32)
        ok = fine & (E != 0)
        eq = trellis(ys, w, h, E, **mutant)
    soft = np.where(ok[:, None], eq, mlse_model.slicer(y.real.astype(F))).astype(F)
    win = np.where(ok, w, WIN_FELL_BACK).astype(np.int32)
    h = np.where(ok[:, None], h, 0).astype(np.complex64)
    return soft, win, h


def access_batch(sps, x, off, length, amp, toa, enable=None, nsoft=148, oracle=None, **mutant):
    """trxsig_mlse_access_batch on packed bursts: dict(soft [B, nsoft], hard, win [B], chan [B, 5], y [B, 148])."""
    o = oracle or oraclebind.Oracle(sps)
    B = len(off)
    amp = np.broadcast_to(np.asarray(amp, np.complex64), (B,)); toa = np.broadcast_to(np.asarray(toa, np.float32), (B,))
    y = np.zeros((B, 148), np.complex64)
    state = np.zeros(B, np.int32)
    for b in range(B):
        if (enable is not None and not enable[b]) or not mlse_model.burst_enabled(sps, int(off[b]), int(length[b]), toa[b]):
            state[b] = WIN_SKIPPED
            continue
        y[b] = mlse_model.symbols(o, x[off[b]:off[b] + length[b]], amp[b], toa[b])
        if length[b] // sps < 148:
            state[b] = WIN_FELL_BACK
    soft, win, h = equalise(y, **mutant)
    short = state == WIN_FELL_BACK
    if short.any():
        soft[short] = mlse_model.slicer(y[short].real)
        win[short] = WIN_FELL_BACK; h[short] = 0
    skip = state == WIN_SKIPPED
    soft[skip] = 0; win[skip] = WIN_SKIPPED; h[skip] = 0
    soft = np.ascontiguousarray(soft[:, :nsoft])
    with np.errstate(all="ignore"):
        hard = (soft > F(0.5)).astype(np.uint8)
    return dict(soft=soft, hard=hard, win=win, chan=h, y=y)
