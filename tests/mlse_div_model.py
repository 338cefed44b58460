"""The float32 model of the two-antenna sequence equaliser (trxsig_mlse_div_batch, csrc/trxsig_mlse_div.hip): the algorithm of
include/trxsig.h restated in numpy float32, operation by operation, vectorised over bursts.  The kernel must equal it word for
word.  It is tests/mlse_model.py with a second antenna: the correlation, the training symbols and the start states are that
module's, the symbols, the window choice, the trellis and the batch wrapper tests/mlse_core.py's; stated here are the tap powers
and the branch metrics summed over the antennas (antenna 0's term first, one float32 addition) and the selection rule.

Every arithmetic step below is ONE float32 operation on float32 arrays, in the order the header states."""
import numpy as np

import mlse_core as core
from mlse_core import F, INF, WIN_FELL_BACK, WIN_SKIPPED  # noqa: F401  (the importers' names)
from mlse_model import (LEFT0, RIGHT0, STEPS, burst_enabled, correlate, inv_amp, slicer, start_states, symbols,  # noqa: F401
                        tsc_symbols)


def estimate(y, t):
    """Step 2 on symbols y [B, 2, 148] (complex64) with training symbols t [26]: (c [B, 2, 9] for d = -4..4, w [B], h [B, 2, 5], E [B])."""
    c0r, c0i = correlate(y[:, 0], t)
    c1r, c1i = correlate(y[:, 1], t)
    p = (c0r * c0r + c0i * c0i) + (c1r * c1r + c1i * c1i)
    w, E = core.window(p)
    c = np.stack([c0r + 1j * c0i, c1r + 1j * c1i], axis=1).astype(np.complex64)
    h = np.stack([core.taps(c[:, 0], w), core.taps(c[:, 1], w)], axis=1)      # one window for both antennas
    return c, w, h, E


def metric(yr, yi, gr, gi):
    """The branch metrics as core.half takes them, summed over the antennas: yr, yi [B, 2, 148]; gr, gi [B, 2, 5]."""
    Z0r, Z0i = core.expected(gr[:, 0], gi[:, 0])
    Z1r, Z1i = core.expected(gr[:, 1], gi[:, 1])
    rows = np.arange(yr.shape[0])

    def at(n):
        dr0 = yr[rows, 0, n][:, None] - Z0r; di0 = yi[rows, 0, n][:, None] - Z0i
        dr1 = yr[rows, 1, n][:, None] - Z1r; di1 = yi[rows, 1, n][:, None] - Z1i
        g = (dr0 * dr0 + di0 * di0) + (dr1 * dr1 + di1 * di1)
        return g
    return at


def _half(yr, yi, w, gr, gi, start, left):
    """One half-burst trellis for every burst: M_0 - M_1 per step, [B, 61].  yr, yi [B, 2, 148]; gr, gi [B, 2, 5]; start [B]."""
    return core.half(metric(yr, yi, gr, gi), w, start, STEPS, LEFT0 if left else RIGHT0, left)


def trellis(y, tsc, w, h, E, primary=None):
    """Steps 3-4 on symbols y [B, 2, 148] with given windows w [B], taps h [B, 2, 5] and energies E [B]: soft [B, 148] float32 (the
    demodulator's formula on the primary antenna on 61..86)."""
    y = np.ascontiguousarray(y, np.complex64)
    B = y.shape[0]
    primary = np.zeros(B, np.int64) if primary is None else np.asarray(primary, np.int64)
    yr, yi = y.real.astype(F), y.imag.astype(F)
    hr, hi = h.real.astype(F), h.imag.astype(F)
    start_r, start_l = start_states(tsc_symbols(tsc), B)
    with np.errstate(all="ignore"):
        Dr = _half(yr, yi, w, hr, hi, start_r, False)
        Dl = _half(yr, yi, w, hr[:, :, ::-1], hi[:, :, ::-1], start_l, True)
        den = (F(8.0) * E.astype(F))[:, None]
        sr = core.soft_out(Dr, den)
        sl = core.soft_out(Dl, den)
    soft = slicer(yr[np.arange(B), primary])
    soft[:, RIGHT0:148] = sr
    soft[:, LEFT0::-1] = sl                                   # step i is symbol 60 - i
    return soft.astype(F)


def equalise(y, tsc, primary=None):
    """Steps 2-5 on symbols y [B, 2, 148]: (soft [B, 148] float32, win [B] int32 (w, or 1 = fell back), h [B, 2, 5] complex64 (zeros
    on fallback))."""
    y = np.ascontiguousarray(y, np.complex64)
    B = y.shape[0]
    primary = np.zeros(B, np.int64) if primary is None else np.asarray(primary, np.int64)
    fine, ys = core.usable(y)                                 # either antenna's
    with np.errstate(all="ignore"):
        _, w, h, E = estimate(ys, tsc_symbols(tsc))
        ok = fine & (E != 0)
        eq = trellis(ys, tsc, w, h, E, primary)
    return core.fall_back(ok, eq, y[np.arange(B), primary], w, h)


def mlse_div_batch(sps, x0, off0, x1, off1, length, tsc, amp, toa, primary=None, enable=None, nsoft=148, oracle=None):
    """trxsig_mlse_div_batch on packed bursts: dict(soft [B, nsoft], hard, win [B], chan [B, 2, 5], y [B, 2, 148])."""
    return core.batch(lambda y, primary: equalise(y, tsc, primary), sps, [x0, x1], [off0, off1], length, amp, toa, primary=primary,
                      enable=enable, nsoft=nsoft, oracle=oracle)


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
