"""The float32 model of the sequence equaliser for synchronisation bursts (trxsig_mlse_sch_batch, csrc/trxsig_mlse_sch.hip): the
algorithm of include/trxsig.h restated in numpy float32, operation by operation, vectorised over bursts.  The kernel must equal
it word for word.

Every arithmetic step below is ONE float32 operation on float32 arrays, in the order the header states.  The symbols, the tap
loop, the window choice, the trellis and the batch wrapper are tests/mlse_core.py's, the one-antenna branch metric
tests/mlse_model.py's; the exact-integer route to the least-squares table is tests/mlse_access_model.py's; the table itself is
derived here from the extended training sequence and must equal the committed one (csrc/trxsig_mlse_sch_tab.h) word for word.
"""
import functools

import numpy as np

import mlse_access_model
import mlse_core as core
import mlse_model
from fectxbind import XTS_BITS
from mlse_core import F, INF, WIN_FELL_BACK, WIN_SKIPPED  # noqa: F401  (the importers' names)

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
    """(N [9][56], det) of the synchronisation burst's design matrix (mlse_access_model.pinv_integers_of)."""
    return mlse_access_model.pinv_integers_of(design_matrix())


@functools.lru_cache(maxsize=None)
def pinv_table():
    """P32 [9, 56] float32 (mlse_access_model.pinv_table_of)."""
    return mlse_access_model.pinv_table_of(*pinv_integers())


def estimate(y, P32=None):
    """Step 2 on symbols y [B, 148] (complex64): (c [B, 9] for d = -4..4, w [B], h [B, 5], E [B])."""
    P = pinv_table() if P32 is None else np.asarray(P32, F)
    return mlse_model.chosen(*core.ls_estimate(y, P, ROW0))


def half(yr, yi, w, gr, gi, start, left, steps=STEPS, right0=RIGHT0, left0=LEFT0, force_tail=True):
    """One half-burst trellis for every burst: M_0 - M_1 per step, [B, steps].  yr, yi [B, 148]; gr, gi [B, 5]; start [B].
    Step i is symbol right0 + i on y[right0 + i + w] (right) or left0 - i on y[left0 - i + 4 + w] (left); the last three steps are
    tail symbols."""
    return core.half(mlse_model.metric(yr, yi, gr, gi), w, start, steps, left0 if left else right0, left, force_tail)


def trellis(y, w, h, E, start_right=START_RIGHT, start_left=START_LEFT, force_tail=True, reverse_left=True):
    """Steps 3-4 on symbols y [B, 148] with given windows, taps and energies: soft [B, 148] float32 (the demodulator's formula on
    42..105).  start_right / start_left / force_tail / reverse_left: the mutants of tests/test_mlse_sch_model.py."""
    y = np.ascontiguousarray(y, np.complex64)
    yr, yi = y.real.astype(F), y.imag.astype(F)
    hr, hi = h.real.astype(F), h.imag.astype(F)
    lr, li = (hr[:, ::-1], hi[:, ::-1]) if reverse_left else (hr, hi)
    with np.errstate(all="ignore"):
        Dr = half(yr, yi, w, hr, hi, start_right, False, force_tail=force_tail)
        Dl = half(yr, yi, w, lr, li, start_left, True, force_tail=force_tail)
        den = (F(8.0) * E.astype(F))[:, None]
        sr = core.soft_out(Dr, den)
        sl = core.soft_out(Dl, den)
    soft = mlse_model.slicer(yr)
    soft[:, RIGHT0:RIGHT0 + STEPS] = sr
    soft[:, LEFT0::-1] = sl                                   # step i is symbol 41 - i
    return soft.astype(F)


def equalise(y, **mutant):
    """Steps 2-5 on symbols y [B, 148]: (soft [B, 148] float32, win [B] int32 (w, or 1 = fell back), h [B, 5] complex64)."""
    y = np.ascontiguousarray(y, np.complex64)
    P32 = mutant.pop("P32", None)
    fine, ys = core.usable(y)
    with np.errstate(all="ignore"):
        _, w, h, E = estimate(ys, P32)
        ok = fine & (E != 0)
        eq = trellis(ys, w, h, E, **mutant)
    return core.fall_back(ok, eq, y, w, h)


def sch_batch(sps, x, off, length, amp, toa, enable=None, nsoft=148, oracle=None, **mutant):
    """trxsig_mlse_sch_batch on packed bursts: dict(soft [B, nsoft], hard, win [B], chan [B, 5], y [B, 148])."""
    return core.batch(lambda y, primary: equalise(y, **mutant), sps, [x], [off], length, amp, toa, enable=enable, nsoft=nsoft, oracle=oracle)
