"""The float64 reference of the synchronisation-burst sequence equaliser (trxsig_mlse_sch_batch): step 3 of the header's comment read
as a statement about SEQUENCES -- no states, no predecessors, no alpha or beta -- and step 2 as a plain least-squares solve.
tests/mlse_sch_model.py and the kernel are graded against it (tests/test_mlse_sch_model.py, tests/test_gpu_mlse_sch_ref.py).  What
is general in tests/mlse_ref.py is used from there (the factor tables of a chain with its known symbols pinned, its exact
min-marginals, the sums P and Q, the three conditions); nothing is shared with the model or the kernel.

The operation.  With the burst model y[n] = sum_k h[k] a[n - w - k], a[n] = +-1, the soft bit of symbol m is
    soft64[m] = 0.5 + (M_0 - M_1) / (8 E64),       E64 = sum_k |h[k]|^2,
where M_b is the minimum, over every symbol sequence that agrees with the known symbols and has bit m = b, of the summed squared
error.  The two halves, in absolute symbol indices (x[i] = a[42 + i] is the extended training sequence):
    right   variables a[102..147]; one term |y[m + w] - sum_k h[k] a[m - k]|^2 per m = 106..147;
            a[102..105] = x[60..63], a[145..147] = -1;
    left    variables a[0..45]; one term |y[m + 4 + w] - sum_k h[k] a[m + 4 - k]|^2 per m = 0..41;
            a[42..45] = x[0..3], a[0..2] = -1.
Each half is a chain of 46 binary variables with 42 factors of 32 entries.

The bound on |soft32 - clamp(soft64)| is tests/mlse_ref.py's derivation with L = 42 steps where it has 61; u = 2^-24.  The branch
metric's rounding q(g) does not depend on the number of steps.  A forward metric after step i is off by <= u sum_{j <= i} q_j +
(i + 1) u P (one rounded addition of a value <= P per step), a backward one by <= u sum_{j > i} q_j + (L - 1 - i) u P, and
T = alpha + beta rounds once more: |T32 - T| <= u (Q + (L + 1) P) = u (Q + 43 P), and so is each M_b.  D = M_0 - M_1 rounds once:
|D32 - D| <= 2 u (Q + 43 P) + u |D|.  The quotient and the last addition are as there (E32 is five two-rounding products and four
additions: E32 = E64 (1 + e), |e| <= 6 u; 4 u + u inside [0, 1], exact clamps beyond), per burst and half:
        bound = 1.001 * ((2 Q + 2 (L + 1) P) / (8 E64) + 5) * u,      2 (L + 1) = 86.

The estimator.  c64 = the least-squares solution of A c = y[46..101] in float64 (numpy's lstsq on the 56 x 9 matrix of +-1: no
table).  The float32 taps are c32[d] = fl(sum_j P32[d][j] y[46 + j]) with 56 products and 55 roundings of partial sums (the first
addition, to 0, is exact).  With Ymax the largest component magnitude among y[46..101] and S1[d] = sum_j |P32[d][j]|:
  * the table: P32 = P (1 + r), |r| <= u (the double division's own 2^-53 is inside the slack): sum_j |P32 - P| |y| <= u S1 Ymax (1 + u);
  * each product rounds once, u |P32 y|: in sum <= u S1 Ymax;
  * each of the 55 additions rounds a partial sum of magnitude <= S1 Ymax (1 + 55 u): in sum <= 55 u S1 Ymax;
  * the float64 solve itself is good to about cond(A) 2^-53 |c|, covered by the slack.
        |c32[d] - c64[d]| <= tol_c[d] = 1.001 * 57 u S1[d] Ymax     per component.
S1 is 1.0000 for every row (at most 56 * 0.0253 = 1.42 from the entries' size alone), so the bound is 57 u Ymax: the access burst's
is about 45 u Ymax, the normal burst's 16 u Ymax.  The window's tolerance follows from tol_c as in tests/mlse_ref.py.
Nothing here was fitted to an observed error.
"""
import numpy as np

import mlse_ref
from fectxbind import XTS_BITS
from mlse_ref import SLACK, U

STEPS = 42
RIGHT = np.arange(106, 148)
LEFT = np.arange(0, 42)
TRELLIS = np.r_[LEFT, RIGHT]
K_P = 2.0 * (STEPS + 1)                                       # the factor of P in the bound: 86
K_C = 57.0                                                    # the factor of u S1 Ymax in the tap bound: 1 + 1 + 55
ROWS = np.arange(46, 102)                                     # the positions the estimator reads
XTS = np.array([int(v) for v in XTS_BITS], np.int64)          # x[i] = bit 42 + i


def half_tables(y, w, h, left):
    """The factor tables of one half, [B, 42, 32], with the known symbols pinned, and (dr, di) for the bound.  Chain variable v is
    a[first + v]; factor l covers a[first + l .. first + l + 4], the newest of them against tap h[0]."""
    if left:
        first, n = 0, LEFT + 4                                              # m = 0..41 reads y[m + 4 + w]; factor m covers a[m..m+4]
        known = {42 + i: int(XTS[i]) for i in range(4)}
        known.update({0: 0, 1: 0, 2: 0})
    else:
        first, n = 102, RIGHT                                               # m = 106..147 reads y[m + w]; factor m - 106 covers a[m-4..m]
        known = {42 + i: int(XTS[i]) for i in range(60, 64)}
        known.update({145: 0, 146: 0, 147: 0})
    return mlse_ref.chain_tables(y, w, h, n, first, known) + (first,)


def equalise64(y, w, h):
    """The reference on symbols y [B, 148] (complex64), windows w [B] and taps h [B, 5] (complex64): dict(soft [B, 148] float64,
    unclamped, NaN on 42..105; bound [B, 148] (per half; NaN on 42..105); E [B]; P, Q [B, 2], right and left)."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    h = np.ascontiguousarray(h, np.complex64).astype(np.complex128)
    w = np.asarray(w, np.int64)
    assert y.ndim == 2 and y.shape[1] == 148 and h.shape == (y.shape[0], 5) and np.all((w >= -4) & (w <= 0))
    B = y.shape[0]
    E = (h.real ** 2 + h.imag ** 2).sum(axis=1)
    soft = np.full((B, 148), np.nan); bound = np.full((B, 148), np.nan)
    P = np.zeros((B, 2)); Q = np.zeros((B, 2))
    for left in (False, True):
        tab, dr, di, first = half_tables(y, w, h, left)
        mm = mlse_ref.min_marginals(tab)                      # [B, 46, 2]
        ms = LEFT if left else RIGHT
        D = mm[:, ms - first, 0] - mm[:, ms - first, 1]       # minmarg[a[m] = -1] - minmarg[a[m] = +1]
        soft[:, ms] = 0.5 + D / (8.0 * E[:, None])
        P[:, int(left)], Q[:, int(left)] = mlse_ref.bound_terms(tab, dr, di, h)
        bound[:, ms] = (SLACK * ((2.0 * Q[:, int(left)] + K_P * P[:, int(left)]) / (8.0 * E) + 5.0) * U)[:, None]
    return dict(soft=soft, bound=bound, E=E, P=P, Q=Q)


def estimate64(y, P32):
    """The estimator in float64 on symbols y [B, 148]: dict(c [B, 9] for d = -4..4; E [B, 5], E[:, q] the energy of window w = -q;
    tol_c [B, 9], the bound on |c32 - c64| per component; tol_E [B], how far below the largest the chosen window's E64 may lie).
    P32 (the float32 table the taps were formed with) enters the BOUND only, through its row sums."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    a = {42 + i: 2.0 * XTS[i] - 1.0 for i in range(64)}
    A = np.array([[a[n - d] for d in range(-4, 5)] for n in ROWS])
    c = np.linalg.lstsq(A, y[:, ROWS].T, rcond=None)[0].T
    p = c.real ** 2 + c.imag ** 2
    E = np.stack([p[:, 4 - q:9 - q].sum(axis=1) for q in range(5)], axis=1)
    ymax = np.maximum(np.abs(y[:, ROWS].real), np.abs(y[:, ROWS].imag)).max(axis=1)
    S1 = np.abs(np.asarray(P32, np.float64)).sum(axis=1)
    e = SLACK * K_C * U * S1[None, :] * ymax[:, None]
    per = 2.0 * (np.abs(c.real) + np.abs(c.imag)) * e + 2.0 * e ** 2
    tau = np.stack([per[:, 4 - q:9 - q].sum(axis=1) for q in range(5)], axis=1) + 6.0 * U * E
    return dict(c=c, E=E, tol_c=e, tol_E=SLACK * 2.0 * tau.max(axis=1))


def grade(soft, hard, y, w, h, ref=None):
    """tests/mlse_ref.py's three conditions on soft [B, 148] float32 and hard [B, 148] against the reference on (y, w, h), on the
    positions 0..41 and 106..147: bad_soft, bad_clamp, bad_hard, excluded, ratio (see there).  The reference alone decides
    `excluded`."""
    return mlse_ref.graded(soft, hard, ref or equalise64(y, w, h), TRELLIS)


def check(soft, hard, y, w, h, what):
    """Assert the three conditions (grade).  Returns grade's dict."""
    return mlse_ref.checked(grade(soft, hard, y, w, h), soft, hard, what)
