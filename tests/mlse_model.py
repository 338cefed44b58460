"""The float32 model of the sequence equaliser (trxsig_mlse_batch, csrc/trxsig_mlse.hip): the algorithm of include/trxsig.h
restated in numpy float32, operation by operation, vectorised over bursts.  The kernel must equal it word for word.

Every arithmetic step below is ONE float32 operation on float32 arrays (numpy rounds each separately; nothing here is a
float64 intermediate), in the order the header states.  What every equaliser model shares is tests/mlse_core.py's, called from
here: the symbols, the slicer, the window choice, the expected values, the trellis, the soft-bit formula and the batch wrapper.
This file keeps the normal burst's own: the 16-term correlation, the one-antenna branch metric (the access and synchronisation
bursts' models use it from here), the start states after the training sequence and the two halves' positions.
"""
import numpy as np

import mlse_core as core
import synth
from mlse_core import F, INF, WIN_FELL_BACK, WIN_SKIPPED, burst_enabled, inv_amp, slicer, symbols  # noqa: F401  (the importers' names)

STEPS, RIGHT0, LEFT0 = 61, 87, 60                             # per half; the first symbol each half decides (the left walks down to 0)


def tsc_symbols(tsc):
    """t[j] = a[61 + j] = 2 bit - 1, float32 [26]."""
    return (2.0 * np.array([int(ch) for ch in synth.TRAINING_SEQUENCE[tsc]], np.float32) - 1.0).astype(F)


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
    """Step 2 on symbols y [B, 148] (complex64) with training symbols t [26]: (c [B, 9] for d = -4..4, w [B], h [B, 5], E [B])."""
    cr, ci = correlate(y, t)
    return chosen(cr, ci)


def chosen(cr, ci):
    """Step 2 from one antenna's nine taps on: (c [B, 9] complex64, w [B], h [B, 5], E [B])."""
    w, E = core.window(cr * cr + ci * ci)
    c = (cr + 1j * ci).astype(np.complex64)
    return c, w, core.taps(c, w), E


def start_states(t, B):
    """(right, left) [B]: the states the training symbols t [26] leave, the newest symbol in bit 0."""
    bit = (t > 0).astype(np.int64)
    start_r = np.full(B, bit[25] | (bit[24] << 1) | (bit[23] << 2) | (bit[22] << 3))
    start_l = np.full(B, bit[0] | (bit[1] << 1) | (bit[2] << 2) | (bit[3] << 3))
    return start_r, start_l


def metric(yr, yi, gr, gi):
    """One antenna's branch metrics as core.half takes them: of the step that reads sample n [B], |y[n] - Z[x]|^2, [B, 32]."""
    Zr, Zi = core.expected(gr, gi)
    rows = np.arange(yr.shape[0])

    def at(n):
        dr = yr[rows, n][:, None] - Zr; di = yi[rows, n][:, None] - Zi
        g = dr * dr + di * di
        return g
    return at


def _half(yr, yi, w, gr, gi, start, left):
    """One half-burst trellis for every burst: M_0 - M_1 per step, [B, 61].  yr, yi [B, 148]; gr, gi [B, 5]; start [B]."""
    return core.half(metric(yr, yi, gr, gi), w, start, STEPS, LEFT0 if left else RIGHT0, left)


def trellis(y, tsc, w, h, E):
    """Steps 3-4 on symbols y [B, 148] with given windows w [B], taps h [B, 5] and energies E [B]: soft [B, 148] float32 (the
    demodulator's formula on 61..86)."""
    y = np.ascontiguousarray(y, np.complex64)
    yr, yi = y.real.astype(F), y.imag.astype(F)
    hr, hi = h.real.astype(F), h.imag.astype(F)
    start_r, start_l = start_states(tsc_symbols(tsc), y.shape[0])
    with np.errstate(all="ignore"):
        Dr = _half(yr, yi, w, hr, hi, start_r, False)
        Dl = _half(yr, yi, w, hr[:, ::-1], hi[:, ::-1], start_l, True)
        den = (F(8.0) * E.astype(F))[:, None]
        sr = core.soft_out(Dr, den)
        sl = core.soft_out(Dl, den)
    soft = slicer(yr)
    soft[:, RIGHT0:148] = sr
    soft[:, LEFT0::-1] = sl                                   # step i is symbol 60 - i
    return soft.astype(F)


def equalise(y, tsc):
    """Steps 2-5 on symbols y [B, 148]: (soft [B, 148] float32, win [B] int32 (w, or 1 = fell back), h [B, 5] complex64 (zeros on fallback))."""
    y = np.ascontiguousarray(y, np.complex64)
    fine, ys = core.usable(y)
    with np.errstate(all="ignore"):
        _, w, h, E = estimate(ys, tsc_symbols(tsc))
        ok = fine & (E != 0)
        eq = trellis(ys, tsc, w, h, E)
    return core.fall_back(ok, eq, y, w, h)


def mlse_batch(sps, x, off, length, tsc, amp, toa, enable=None, nsoft=148, oracle=None):
    """trxsig_mlse_batch on packed bursts: dict(soft [B, nsoft], hard, win [B], chan [B, 5], y [B, 148])."""
    return core.batch(lambda y, primary: equalise(y, tsc), sps, [x], [off], length, amp, toa, enable=enable, nsoft=nsoft, oracle=oracle)
