"""The float64 reference of the access-burst sequence equaliser (trxsig_mlse_access_batch): step 3 of the header's comment read as a
statement about SEQUENCES -- no states, no predecessors, no alpha or beta -- and step 2 as a plain least-squares solve.
tests/mlse_access_model.py and the kernel are graded against it (tests/test_mlse_access_model.py,
tests/test_gpu_mlse_access_ref.py).  What is general in tests/mlse_ref.py is used from there (the factor tables of a chain with
its known symbols pinned, its exact min-marginals, the sums P and Q, the three conditions); nothing is shared with the model or the kernel.

The operation.  With the burst model y[n] = sum_k h[k] a[n - w - k], a[n] = +-1, the soft bit of symbol m = 49..87 is
    soft64[m] = 0.5 + (M_0 - M_1) / (8 E64),       E64 = sum_k |h[k]|^2,
where M_b is the minimum, over every symbol sequence that agrees with the known symbols and has bit m = b, of the summed squared
error: variables a[45..87]; one term |y[m + w] - sum_k h[k] a[m - k]|^2 per m = 49..87; a[45..48] = the last four bits of the
synchronisation sequence, a[85..87] = -1.  A chain of 43 binary variables with 39 factors of 32 entries.

The bound on |soft32 - clamp(soft64)| is tests/mlse_ref.py's derivation with L = 39 steps where it has 61; u = 2^-24.  The branch
metric's rounding q(g) does not depend on the number of steps.  A forward metric after step i is off by <= u sum_{j <= i} q_j +
(i + 1) u P (one rounded addition of a value <= P per step), a backward one by <= u sum_{j > i} q_j + (L - 1 - i) u P, and
T = alpha + beta rounds once more: |T32 - T| <= u (Q + (L + 1) P) = u (Q + 40 P), and so is each M_b.  D = M_0 - M_1 rounds once:
|D32 - D| <= 2 u (Q + 40 P) + u |D|.  The quotient and the last addition are as there (E32 is five two-rounding products and four
additions: E32 = E64 (1 + e), |e| <= 6 u; 4 u + u inside [0, 1], exact clamps beyond):
        bound = 1.001 * ((2 Q + 2 (L + 1) P) / (8 E64) + 5) * u,      2 (L + 1) = 80.

The estimator.  c64 = the least-squares solution of A c = y[4..44] in float64 (numpy's lstsq on the 41 x 9 matrix of +-1: no table).
The float32 taps are c32[d] = fl(sum_j P32[d][j] y[4 + j]) with 41 products and 40 roundings of partial sums (the first addition,
to 0, is exact).  With Ymax the largest component magnitude among y[4..44] and S1[d] = sum_j |P32[d][j]|:
  * the table: P32 = P (1 + r), |r| <= u (the double division's own 2^-53 is inside the slack): sum_j |P32 - P| |y| <= u S1 Ymax (1 + u);
  * each product rounds once, u |P32 y|: in sum <= u S1 Ymax;
  * each of the 40 additions rounds a partial sum of magnitude <= S1 Ymax (1 + 40 u): in sum <= 40 u S1 Ymax;
  * the float64 solve itself is good to about cond(A) 2^-53 |c|, covered by the slack.
        |c32[d] - c64[d]| <= tol_c[d] = 1.001 * 42 u S1[d] Ymax     per component.
S1 is at most 41 * 0.04 = 1.64 (1.0 to 1.1 in fact), so the bound is about 45 u Ymax: three times the normal burst's 16 u Ymax.
Nothing here was fitted to an observed error.
"""
import numpy as np

import l1_ms_model as lms
import mlse_ref
from mlse_ref import SLACK, U

FIRST, STEPS = 49, 39
TRELLIS = np.arange(FIRST, FIRST + STEPS)
K_P = 2.0 * (STEPS + 1)                                       # the factor of P in the bound: 80


def factor_tables(y, w, h):
    """The factor tables [B, 39, 32] with the known symbols pinned, and (dr, di) for the bound.  Chain variable v is a[45 + v];
    factor l covers a[45 + l .. 49 + l], the newest of them against tap h[0]."""
    first = FIRST - 4
    known = {m: int(lms.ACCESS_HEAD[m]) for m in range(45, 49)}
    known.update({85: 0, 86: 0, 87: 0})
    return mlse_ref.chain_tables(y, w, h, TRELLIS, first, known) + (first,)


def equalise64(y, w, h):
    """The reference on symbols y [B, 148] (complex64), windows w [B] and taps h [B, 5] (complex64): dict(soft [B, 148] float64,
    unclamped, NaN off 49..87; bound [B, 148]; E, P, Q [B])."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    h = np.ascontiguousarray(h, np.complex64).astype(np.complex128)
    w = np.asarray(w, np.int64)
    assert y.ndim == 2 and y.shape[1] == 148 and h.shape == (y.shape[0], 5) and np.all((w >= -4) & (w <= 0))
    B = y.shape[0]
    E = (h.real ** 2 + h.imag ** 2).sum(axis=1)
    soft = np.full((B, 148), np.nan); bound = np.full((B, 148), np.nan)
    tab, dr, di, first = factor_tables(y, w, h)
    mm = mlse_ref.min_marginals(tab)                          # [B, 43, 2]
    D = mm[:, TRELLIS - first, 0] - mm[:, TRELLIS - first, 1]
    soft[:, TRELLIS] = 0.5 + D / (8.0 * E[:, None])
    P, Q = mlse_ref.bound_terms(tab, dr, di, h)
    bound[:, TRELLIS] = (SLACK * ((2.0 * Q + K_P * P) / (8.0 * E) + 5.0) * U)[:, None]
    return dict(soft=soft, bound=bound, E=E, P=P, Q=Q)


def estimate64(y, P32):
    """The estimator in float64 on symbols y [B, 148]: dict(c [B, 9] for d = -4..4; E [B, 5], E[:, q] the energy of window w = -q;
    tol_c [B, 9], the bound on |c32 - c64| per component; tol_E [B], how far below the largest the chosen window's E64 may lie).
    P32 (the float32 table the taps were formed with) enters the BOUND only, through its row sums."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    head = 2.0 * lms.ACCESS_HEAD.astype(np.float64) - 1.0
    A = np.array([[head[n - d] for d in range(-4, 5)] for n in range(4, 45)])
    c = np.linalg.lstsq(A, y[:, 4:45].T, rcond=None)[0].T
    p = c.real ** 2 + c.imag ** 2
    E = np.stack([p[:, 4 - q:9 - q].sum(axis=1) for q in range(5)], axis=1)
    ymax = np.maximum(np.abs(y[:, 4:45].real), np.abs(y[:, 4:45].imag)).max(axis=1)
    S1 = np.abs(np.asarray(P32, np.float64)).sum(axis=1)
    e = SLACK * 42.0 * U * S1[None, :] * ymax[:, None]
    per = 2.0 * (np.abs(c.real) + np.abs(c.imag)) * e + 2.0 * e ** 2
    tau = np.stack([per[:, 4 - q:9 - q].sum(axis=1) for q in range(5)], axis=1) + 6.0 * U * E
    return dict(c=c, E=E, tol_c=e, tol_E=SLACK * 2.0 * tau.max(axis=1))


def grade(soft, hard, y, w, h, ref=None):
    """tests/mlse_ref.py's three conditions on soft [B, 148] float32 and hard [B, 148] against the reference on (y, w, h), on the
    positions 49..87: bad_soft, bad_clamp, bad_hard, excluded, ratio (see there).  The reference alone decides `excluded`."""
    return mlse_ref.graded(soft, hard, ref or equalise64(y, w, h), TRELLIS)


def check(soft, hard, y, w, h, what):
    """Assert the three conditions (grade).  Returns grade's dict."""
    return mlse_ref.checked(grade(soft, hard, y, w, h), soft, hard, what)
