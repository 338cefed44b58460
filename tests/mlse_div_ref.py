"""The float64 reference of the two-antenna sequence equaliser (trxsig_mlse_div_batch): tests/mlse_ref.py's statement about
SEQUENCES with the squared error summed over both antennas.  tests/mlse_div_model.py and the kernel are graded against it
(tests/test_mlse_div_model.py, tests/test_gpu_mlse_div.py); nothing here is imported from, or shared with, either.

The operation.  With the burst model y_a[n] = sum_k h_a[k] a[n - w - k] on antenna a = 0, 1 (one window w, one symbol sequence),
    soft64[m] = 0.5 + (M_0 - M_1) / (8 E64),       E64 = sum_a sum_k |h_a[k]|^2,
where M_b is the minimum, over every symbol sequence that agrees with the known symbols and has bit m = b, of the squared error
summed over the steps AND the antennas.  Per half that is mlse_ref's chain with the factor table tab_0 + tab_1
(mlse_ref.half_tables per antenna, the same pinned entries in both), and M_b its min-marginal (mlse_ref.min_marginals).  Inputs
are the float32 symbols y [2, 148], the window and the 2 x 5 float32 taps, widened to float64.

The bound on |soft32 - clamp(soft64)|, u = 2^-24, to first order in u (1.001 covers the rest, as in mlse_ref).  mlse_ref's
derivation with the roundings that are added:
  * One summed branch metric.  Each antenna's metric is off by u q(g_a), q(g_a) = 4 g_a + 8 (|dr_a| Sr_a + |di_a| Si_a) with that
    antenna's Sr_a = sum_k |Re h_a[k]|, Si_a (mlse_ref.bound_terms).  Their float32 sum rounds once more, by u (g_0 + g_1):
        |gamma32 - gamma| <= u (q(g_0) + q(g_1) + (g_0 + g_1)) =: u q2.
  * Sums.  G_i = the largest finite summed metric of step i, P = sum_i G_i; Q = sum_i max_x q2 over the finite branches of step i.
    alpha, beta, T and M_b are word for word mlse_ref's on these numbers: |T32 - T| <= u (Q + 62 P), and so is each M_b;
    |D32 - D| <= 2 u (Q + 62 P) + u |D|.
  * The quotient.  p[d] is two products-and-sums (2 u relative each, both positive) and ONE MORE addition: 3 u relative where the
    one-antenna p[d] has 2 u; the four additions of a window add 4 u: E32 = E64 (1 + e), |e| <= 7 u where mlse_ref has 6 u.
    8 E32 is exact, the division rounds once: |D32 / (8 E32) - D / (8 E64)| <= 2 u (Q + 62 P) / (8 E64) + 9 u |D / (8 E64)|.
    The last addition rounds u |soft|.  Where soft64 lies in [0, 1], |D / (8 E64)| <= 1/2: the two last terms are <= 4.5 u + u
    = 5.5 u, taken as 6 u (mlse_ref: 4 u + u = 5 u).  Outside [0, 1] by t the terms grow by 10 u t while the distance to the clamp
    grows by t, and the clamp is 1-Lipschitz: the same bound holds against clamp(soft64).
        bound = 1.001 * ((2 Q + 124 P) / (8 E64) + 6) * u
Nothing here was fitted to an observed error."""
import numpy as np

import mlse_ref

U = mlse_ref.U
SLACK = mlse_ref.SLACK
TRELLIS = mlse_ref.TRELLIS


def equalise64(y, w, h, tsc):
    """The reference on symbols y [B, 2, 148] (complex64), windows w [B] and taps h [B, 2, 5] (complex64): dict(soft [B, 148]
    float64, unclamped, NaN on 61..86; bound [B, 148] (per half; NaN on 61..86); E [B]; P, Q [B, 2], right and left)."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    h = np.ascontiguousarray(h, np.complex64).astype(np.complex128)
    w = np.asarray(w, np.int64)
    B = y.shape[0]
    assert y.shape == (B, 2, 148) and h.shape == (B, 2, 5) and np.all((w >= -4) & (w <= 0))
    E = (h.real ** 2 + h.imag ** 2).sum(axis=(1, 2))
    soft = np.full((B, 148), np.nan); bound = np.full((B, 148), np.nan)
    P = np.zeros((B, 2)); Q = np.zeros((B, 2))
    for left in (False, True):
        tab = 0.0; q = 0.0
        for a in (0, 1):
            ta, dr, di, first = mlse_ref.half_tables(y[:, a], w, h[:, a], tsc, left)
            Sr = np.abs(h[:, a].real).sum(axis=1)[:, None, None]; Si = np.abs(h[:, a].imag).sum(axis=1)[:, None, None]
            fin = np.isfinite(ta)
            q = q + np.where(fin, 4.0 * ta + 8.0 * (np.abs(dr) * Sr + np.abs(di) * Si), 0.0)      # q(g_a); the pinned entries are the same in both
            tab = tab + ta
        fin = np.isfinite(tab)
        g = np.where(fin, tab, 0.0)
        q = np.where(fin, q + g, 0.0)                          # ... + (g_0 + g_1): the sum's own rounding
        mm = mlse_ref.min_marginals(tab)                       # [B, 65, 2]
        ms = np.arange(0, 61) if left else np.arange(87, 148)
        D = mm[:, ms - first, 0] - mm[:, ms - first, 1]
        soft[:, ms] = 0.5 + D / (8.0 * E[:, None])
        P[:, int(left)] = g.max(axis=2).sum(axis=1); Q[:, int(left)] = q.max(axis=2).sum(axis=1)
        bound[:, ms] = (SLACK * ((2.0 * Q[:, int(left)] + 124.0 * P[:, int(left)]) / (8.0 * E) + 6.0) * U)[:, None]
    return dict(soft=soft, bound=bound, E=E, P=P, Q=Q)


def grade(soft, hard, y, w, h, tsc):
    """mlse_ref.grade's three conditions (bad_soft, bad_clamp, bad_hard), `excluded` and `ratio` on soft [B, 148] float32 and hard
    [B, 148] against this reference on (y [B, 2, 148], w, h [B, 2, 5]).  The reference alone decides `excluded`."""
    return mlse_ref.graded(soft, hard, equalise64(y, w, h, tsc), TRELLIS)


def check(soft, hard, y, w, h, tsc, what):
    """Assert the three conditions; returns grade's dict."""
    return mlse_ref.checked(grade(soft, hard, y, w, h, tsc), soft, hard, what)
