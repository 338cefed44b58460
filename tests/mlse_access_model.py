"""The float32 model of the sequence equaliser for access bursts (trxsig_mlse_access_batch, csrc/trxsig_mlse_access.hip): the
algorithm of include/trxsig.h restated in numpy float32, operation by operation, vectorised over bursts.  The kernel must equal
it word for word.

Every arithmetic step below is ONE float32 operation on float32 arrays, in the order the header states.  The symbols, the tap
loop, the window choice, the trellis and the batch wrapper are tests/mlse_core.py's, the one-antenna branch metric
tests/mlse_model.py's; the least-squares table is derived here from Python integers and must equal the committed one
(csrc/trxsig_mlse_access_tab.h) word for word.
"""
import functools
from fractions import Fraction

import numpy as np

import l1_ms_model as lms
import mlse_core as core
import mlse_model
from mlse_core import F, INF, WIN_FELL_BACK, WIN_SKIPPED  # noqa: F401  (the importers' names)

NTAP, NROW = 9, 41                                            # c[-4..4]; the positions n = 4..44 whose nine symbols are all known
ROW0 = 4                                                      # the first of them
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


def pinv_integers_of(A):
    """(N [9][rows], det) of a design matrix A [rows][9]: N = adj(A^T A) A^T and det(A^T A), Python integers; the least-squares
    estimator is N / det."""
    nrow = len(A)
    G = [[sum(A[n][i] * A[n][j] for n in range(nrow)) for j in range(NTAP)] for i in range(NTAP)]
    det, adj = _det_adj(G)
    N = [[sum(adj[i][k] * A[n][k] for k in range(NTAP)) for n in range(nrow)] for i in range(NTAP)]
    return N, det


def pinv_table_of(N, det):
    """P32 [9, rows] float32: (float)((double)N / (double)det), one correctly rounded double division of two exactly representable
    integers (Python's int / int is correctly rounded too, and the same here: both are below 2^53), then one rounding to float32."""
    assert abs(det) < 2 ** 53 and all(abs(v) < 2 ** 53 for row in N for v in row)
    P = np.array([[float(v) / float(det) for v in row] for row in N], np.float64).astype(F)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def pinv_integers():
    """(N [9][41], det) of the access burst's design matrix (pinv_integers_of)."""
    return pinv_integers_of(design_matrix())


@functools.lru_cache(maxsize=None)
def pinv_table():
    """P32 [9, 41] float32 (pinv_table_of)."""
    return pinv_table_of(*pinv_integers())


def estimate(y, P32=None):
    """Step 2 on symbols y [B, 148] (complex64): (c [B, 9] for d = -4..4, w [B], h [B, 5], E [B])."""
    P = pinv_table() if P32 is None else np.asarray(P32, F)
    return mlse_model.chosen(*core.ls_estimate(y, P, ROW0))


def trellis(y, w, h, E, start=START, force_tail=True, sign_w=1):
    """Steps 3-4 on symbols y [B, 148] with given windows, taps and energies: soft [B, 148] float32 (the demodulator's formula
    on 0..48 and 88..147).  start / force_tail / sign_w: the mutants of tests/test_mlse_access_model.py."""
    y = np.ascontiguousarray(y, np.complex64)
    yr, yi = y.real.astype(F), y.imag.astype(F)
    with np.errstate(all="ignore"):
        D = core.half(mlse_model.metric(yr, yi, h.real.astype(F), h.imag.astype(F)), w, start, STEPS, FIRST, False, force_tail, sign_w)
        s = core.soft_out(D, (F(8.0) * E.astype(F))[:, None])
    soft = mlse_model.slicer(yr)
    soft[:, FIRST:FIRST + STEPS] = s
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


def access_batch(sps, x, off, length, amp, toa, enable=None, nsoft=148, oracle=None, **mutant):
    """trxsig_mlse_access_batch on packed bursts: dict(soft [B, nsoft], hard, win [B], chan [B, 5], y [B, 148])."""
    return core.batch(lambda y, primary: equalise(y, **mutant), sps, [x], [off], length, amp, toa, enable=enable, nsoft=nsoft, oracle=oracle)
