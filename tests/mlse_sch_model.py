"""The float32 model of the sequence equaliser for synchronisation bursts (trxsig_mlse_sch_batch, csrc/trxsig_mlse_sch.hip): the
algorithm of include/trxsig.h restated in numpy float32, operation by operation, vectorised over bursts.  The kernel must equal
it word for word.

Every arithmetic step below is ONE float32 operation on float32 arrays, in the order the header states.  The symbols, the slicer
and the geometry test are tests/mlse_model.py's; the exact-integer route to the least-squares table is
tests/mlse_access_model.py's (its Gauss-Jordan on Fractions is used from there); the table itself is derived here from the
extended training sequence and must equal the committed one (csrc/trxsig_mlse_sch_tab.h) word for word.

The half-burst trellis: tests/mlse_model.py's _half is written for 61 steps on the normal burst's positions, so it cannot be
called for 42; half() below is the same recursion with the step count and the first position as arguments, and
tests/test_mlse_sch_model.py holds it to _half word for word with the normal burst's numbers put in.
"""
import functools

import numpy as np

import mlse_access_model
import mlse_model
import oraclebind
from fectxbind import XTS_BITS

F = np.float32
INF = F(np.inf)
WIN_FELL_BACK, WIN_SKIPPED = mlse_model.WIN_FELL_BACK, mlse_model.WIN_SKIPPED
NTAP, NROW = 9, 56                                            # c[-4..4]; the positions n = 46..101 whose nine symbols are all known
ROW0 = 46                                                     # the first of them
XTS0, NXTS = 42, 64                                           # a[42 + i] = 2 XTS[i] - 1
STEPS = 42                                                    # per half: 39 coded bits and 3 tail bits
RIGHT0, LEFT0 = 106, 41                                       # the first symbol each half decides (the left half walks down to 0)
XTS = np.array([int(v) for v in XTS_BITS], np.int64)
assert len(XTS) == NXTS


def _state(bits):
    """bit 0 first"""
    return int(bits[0]) | int(bits[1]) << 1 | int(bits[2]) << 2 | int(bits[3]) << 3


START_RIGHT = _state([XTS[105 - XTS0], XTS[104 - XTS0], XTS[103 - XTS0], XTS[102 - XTS0]])     # a[105], a[104], a[103], a[102]
START_LEFT = _state([XTS[0], XTS[1], XTS[2], XTS[3]])                                          # a[42], a[43], a[44], a[45]


def design_matrix():
    """A [56][9] of Python integers: A[n - 46][d + 4] = a[n - d], n = 46..101, d = -4..4."""
    a = {XTS0 + i: 2 * int(XTS[i]) - 1 for i in range(NXTS)}
    return [[a[n - d] for d in range(-4, 5)] for n in range(ROW0, ROW0 + NROW)]


@functools.lru_cache(maxsize=None)
def pinv_integers():
    """(N [9][56], det): N = adj(A^T A) A^T and det(A^T A), Python integers; the least-squares estimator is N / det."""
    A = design_matrix()
    G = [[sum(A[n][i] * A[n][j] for n in range(NROW)) for j in range(NTAP)] for i in range(NTAP)]
    det, adj = mlse_access_model._det_adj(G)
    N = [[sum(adj[i][k] * A[n][k] for k in range(NTAP)) for n in range(NROW)] for i in range(NTAP)]
    return N, det


@functools.lru_cache(maxsize=None)
def pinv_table():
    """P32 [9, 56] float32: (float)((double)N / (double)det), one correctly rounded double division of two exactly representable
    integers (both below 2^53), then one rounding to float32."""
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
            ar = ar + P[k, j] * yr[:, ROW0 + j]
            ai = ai + P[k, j] * yi[:, ROW0 + j]
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


def half(yr, yi, w, gr, gi, start, left, steps=STEPS, right0=RIGHT0, left0=LEFT0, force_tail=True):
    """One half-burst trellis for every burst: M_0 - M_1 per step, [B, steps].  yr, yi [B, 148]; gr, gi [B, 5]; start [B].
    Step i is symbol right0 + i on y[right0 + i + w] (right) or left0 - i on y[left0 - i + 4 + w] (left); the last three steps are
    tail symbols.  tests/mlse_model.py's _half with (61, 87, 60)."""
    B = yr.shape[0]
    x = np.arange(32)
    sign = np.where(((x[:, None] >> np.arange(5)[None, :]) & 1) == 1, F(1.0), F(-1.0)).astype(F)     # [32, 5]
    Zr = gr[:, None, 0] * sign[None, :, 0]; Zi = gi[:, None, 0] * sign[None, :, 0]
    for k in range(1, 5):
        Zr = Zr + gr[:, None, k] * sign[None, :, k]
        Zi = Zi + gi[:, None, k] * sign[None, :, k]
    rows = np.arange(B)
    gam = np.zeros((steps, B, 32), F)
    for i in range(steps):
        n = (left0 - i + 4 + w) if left else (right0 + i + w)
        dr = yr[rows, n][:, None] - Zr; di = yi[rows, n][:, None] - Zi
        g = dr * dr + di * di
        if i >= steps - 3 and force_tail:
            g[:, 1::2] = INF                                   # the tail symbols are -1: b = 1 contradicts
        gam[i] = g
    s = np.arange(16)
    alpha = np.where(s[None, :] == start[:, None], F(0.0), INF).astype(F)
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


def trellis(y, w, h, E, start_right=START_RIGHT, start_left=START_LEFT, force_tail=True, reverse_left=True):
    """Steps 3-4 on symbols y [B, 148] with given windows, taps and energies: soft [B, 148] float32 (the demodulator's formula on
    42..105).  start_right / start_left / force_tail / reverse_left: the mutants of tests/test_mlse_sch_model.py."""
    y = np.ascontiguousarray(y, np.complex64)
    B = y.shape[0]
    yr, yi = y.real.astype(F), y.imag.astype(F)
    hr, hi = h.real.astype(F), h.imag.astype(F)
    lr, li = (hr[:, ::-1], hi[:, ::-1]) if reverse_left else (hr, hi)
    with np.errstate(all="ignore"):
        Dr = half(yr, yi, w, hr, hi, np.full(B, start_right), False, force_tail=force_tail)
        Dl = half(yr, yi, w, lr, li, np.full(B, start_left), True, force_tail=force_tail)
        den = (F(8.0) * E.astype(F))[:, None]
        sr = F(0.5) + Dr / den
        sl = F(0.5) + Dl / den
        sr = np.where(sr > F(1.0), F(1.0), sr); sr = np.where(sr < F(0.0), F(0.0), sr)
        sl = np.where(sl > F(1.0), F(1.0), sl); sl = np.where(sl < F(0.0), F(0.0), sl)
    soft = mlse_model.slicer(yr)
    soft[:, RIGHT0:RIGHT0 + STEPS] = sr
    soft[:, LEFT0::-1] = sl                                   # step i is symbol 41 - i
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


def sch_batch(sps, x, off, length, amp, toa, enable=None, nsoft=148, oracle=None, **mutant):
    """trxsig_mlse_sch_batch on packed bursts: dict(soft [B, nsoft], hard, win [B], chan [B, 5], y [B, 148])."""
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
