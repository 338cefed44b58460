"""The float64 reference of the two-antenna sequence equaliser with interference-rejection combining (trxsig_mlse_irc_batch):
tests/mlse_div_ref.py's statement about SEQUENCES with the whitened squared error.  tests/mlse_irc_model.py and the kernel are
graded against it (tests/test_mlse_irc_model.py, tests/test_gpu_mlse_irc_ref.py); nothing here is imported from, or shared with,
either.

The operation.  Inputs are the float32 symbols y [2, 148], the window, the 2 x 5 float32 taps and the float32 set (A, Bv, xr, xi)
that was used, all widened to float64; everything after them is float64.  x = xr + i xi, det = A Bv - |x|^2,
    y_1'[n] = A y_1[n] - conj(x) y_0[n],    h_1'[k] = A h_1[k] - conj(x) h_0[k],    E64 = sum_k det |h_0[k]|^2 + |h_1'[k]|^2,
    soft64[m] = 0.5 + (M_0 - M_1) / (8 E64),
where M_b is the minimum, over every symbol sequence that agrees with the known symbols and has bit m = b, of
det |d_0|^2 + |d_1'|^2 summed over the steps, d_0 = y_0 - sum_k h_0[k] a[.], d_1' = y_1' - sum_k h_1'[k] a[.].  Per half that is
mlse_ref's chain with the factor table det tab_0 + tab_1' (mlse_ref.half_tables per antenna) and its min-marginals.

The bound on |soft32 - clamp(soft64)|, u = 2^-24, to first order in u (1.001 covers the rest, as in mlse_ref).  It starts from the
float32 roundings alone; mlse_div_ref's derivation with what is added:
  * det.  A Bv rounds u A Bv; xr^2 and xi^2 round u each and their sum once more, 2 u |x|^2; the subtraction u |det|:
        |det32 - det| <= u (A Bv + 2 |x|^2 + |det|) =: u dd.        (Not relative: det may be what a cancellation leaves.)
  * The whitening of a value (v_0, v_1) -> v_1'.  The real part is A v1.re - (xr v0.re + xi v0.im): three products (u each), the
    sum in the parenthesis and the subtraction:
        |v1'32.re - v1'.re| <= u (|A v1.re| + 2 (|xr v0.re| + |xi v0.im|) + |v1'.re|) =: u om_re(v),
    and om_im(v) likewise with (|xr v0.im| + |xi v0.re|).  oy_re[n], oy_im[n] are these for the symbols, oh_re[k], oh_im[k] for the taps.
  * Antenna 0's metric is mlse_ref's: |g_0,32 - g_0| <= u q(g_0), q(g_0) = 4 g_0 + 8 (|dr_0| Sr_0 + |di_0| Si_0).
  * Antenna 1's metric on whitened values.  Z_1' is four float32 additions of +-h_1'32[k]: off from the exact sum of the exact
    h_1'[k] by <= u (4 Sr_1' + sum_k oh_re[k]) =: u W_re (Sr_1' = sum_k |Re h_1'[k]|).  dr_1 = y_1'32.re - Z.re rounds once more:
    |dr32 - dr| <= u |dr| + u (W_re + oy_re[n]).  The square, the other part and their sum as in mlse_ref:
        |g_1,32 - g_1| <= u (4 g_1 + 2 (|dr_1| (W_re + oy_re[n]) + |di_1| (W_im + oy_im[n]))) =: u q1(g_1).
  * The branch metric gamma = det g_0 + g_1.  The product det32 g_0,32 carries det u q(g_0) + u dd g_0 and its own rounding u det g_0;
    the addition rounds u (det g_0 + g_1):
        |gamma32 - gamma| <= u (det q(g_0) + (dd + det) g_0 + q1(g_1) + (det g_0 + g_1)) =: u q3.
  * Sums.  G_i = the largest finite gamma of step i, P = sum_i G_i; Q = sum_i max_x q3 over the finite branches of step i.  alpha,
    beta, T and M_b are word for word mlse_ref's on these numbers: |D32 - D| <= 2 u (Q + 62 P) + u |D|.
  * The quotient.  pw[k] = det |h_0[k]|^2 + |h_1'[k]|^2: |h_0[k]|^2 is 2 u relative, times det32 (u dd absolute) and the product's
    rounding: u |h_0[k]|^2 (3 det + dd); |h_1'32[k]|^2 is off by 2 u (|Re h_1'| oh_re + |Im h_1'| oh_im) + 2 u |h_1'[k]|^2; their
    sum rounds u pw[k]; the four additions of E_w add 4 u E64:
        E32 = E64 (1 + e u'),  e = (sum_k (|h_0[k]|^2 (3 det + dd) + 2 (|Re h_1'[k]| oh_re[k] + |Im h_1'[k]| oh_im[k]) + 2 |h_1'[k]|^2)
                                    + 5 E64) / E64,   |u'| <= u
    (7 in mlse_div_ref, where nothing is whitened; at most 11 for the identity set, whose exact products this derivation still
    counts).  8 E32 is exact, the division rounds once, D itself once:
        |D32 / (8 E32) - D / (8 E64)| <= 2 u (Q + 62 P) / (8 E64) + (e + 2) u |D / (8 E64)|.
    The last addition rounds u |soft|.  Where soft64 lies in [0, 1], |D / (8 E64)| <= 1/2: the two last terms are <= (e / 2 + 2) u.
    Outside [0, 1] by t the terms grow by (e + 3) u t while the distance to the clamp grows by t, and the clamp is 1-Lipschitz: the
    same bound holds against clamp(soft64) as long as (e + 3) u < 1 (asserted).
        bound = 1.001 * ((2 Q + 124 P) / (8 E64) + e / 2 + 2) * u

The residual sums (sums64): S00, S11, Xr, Xi against their float64 sums over the same residual terms -- r_a[m] = y_a[m + w] -
sum_k h_a[k] a[m - k] in float64 from the float32 symbols and taps.
  * A residual.  Z is four float32 additions, the subtraction rounds once more: |r32.re - r.re| <= u (|r.re| + 4 Sr_a) =: u rho_a.re,
    rho_a.im likewise with Si_a.
  * A term.  r0.re^2 + r0.im^2: each square carries 2 |r| u rho and its own rounding, the sum rounds once:
        tau00 = 2 (|r0.re| rho_0.re + |r0.im| rho_0.im) + 2 t00         (tau11 likewise);
    r0.re r1.re + r0.im r1.im: tau_xr = |r1.re| rho_0.re + |r0.re| rho_1.re + |r1.im| rho_0.im + |r0.im| rho_1.im
                                        + 2 (|r0.re r1.re| + |r0.im r1.im|);
    r0.im r1.re - r0.re r1.im: tau_xi = |r1.re| rho_0.im + |r0.im| rho_1.re + |r1.im| rho_0.re + |r0.re| rho_1.im
                                        + 2 (|r0.im r1.re| + |r0.re r1.im|).
  * The sum of 22 terms from 0, m ascending: the first addition is exact, each of the other 21 rounds a partial sum of magnitude
    <= sum_m |t_m|:
        |S32 - S64| <= 1.001 * (sum_m tau_m + 21 sum_m |t_m|) * u
Nothing here was fitted to an observed error."""
import numpy as np

import mlse_ref

U = mlse_ref.U
SLACK = mlse_ref.SLACK
TRELLIS = mlse_ref.TRELLIS


def _omega(A, xr, xi, v0, v1, vw):
    """(om_re, om_im) of the docstring for values v0, v1 and their exact whitened vw; A, xr, xi broadcast against them."""
    o_re = np.abs(A * v1.real) + 2.0 * (np.abs(xr * v0.real) + np.abs(xi * v0.imag)) + np.abs(vw.real)
    o_im = np.abs(A * v1.imag) + 2.0 * (np.abs(xr * v0.imag) + np.abs(xi * v0.real)) + np.abs(vw.imag)
    return o_re, o_im


def equalise64(y, w, h, cov, tsc):
    """The reference on symbols y [B, 2, 148] (complex64), windows w [B], taps h [B, 2, 5] (complex64) and sets cov [B, 4] (float32:
    A, Bv, xr, xi): dict(soft [B, 148] float64, unclamped, NaN on 61..86; bound [B, 148] (per half; NaN on 61..86); E [B]; e [B];
    det [B]; P, Q [B, 2], right and left)."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    h = np.ascontiguousarray(h, np.complex64).astype(np.complex128)
    cov = np.ascontiguousarray(cov, np.float32).astype(np.float64)
    w = np.asarray(w, np.int64)
    B = y.shape[0]
    assert y.shape == (B, 2, 148) and h.shape == (B, 2, 5) and cov.shape == (B, 4) and np.all((w >= -4) & (w <= 0))
    A, Bv, xr, xi = (cov[:, k] for k in range(4))
    x = xr + 1j * xi
    x2 = xr ** 2 + xi ** 2
    det = A * Bv - x2
    assert np.all(det > 0)
    dd = A * Bv + 2.0 * x2 + np.abs(det)
    yw = A[:, None] * y[:, 1] - np.conj(x)[:, None] * y[:, 0]
    hw = A[:, None] * h[:, 1] - np.conj(x)[:, None] * h[:, 0]
    oy_re, oy_im = _omega(A[:, None], xr[:, None], xi[:, None], y[:, 0], y[:, 1], yw)
    oh_re, oh_im = _omega(A[:, None], xr[:, None], xi[:, None], h[:, 0], h[:, 1], hw)
    a0 = h[:, 0].real ** 2 + h[:, 0].imag ** 2; a1 = hw.real ** 2 + hw.imag ** 2
    E = (det[:, None] * a0 + a1).sum(axis=1)
    e = ((a0 * (3.0 * det + dd)[:, None] + 2.0 * (np.abs(hw.real) * oh_re + np.abs(hw.imag) * oh_im) + 2.0 * a1).sum(axis=1) + 5.0 * E) / E
    assert np.all((e + 3.0) * U < 1.0)
    Sr0 = np.abs(h[:, 0].real).sum(axis=1)[:, None, None]; Si0 = np.abs(h[:, 0].imag).sum(axis=1)[:, None, None]
    W_re = 4.0 * np.abs(hw.real).sum(axis=1) + oh_re.sum(axis=1); W_im = 4.0 * np.abs(hw.imag).sum(axis=1) + oh_im.sum(axis=1)
    rows = np.arange(B)[:, None]
    soft = np.full((B, 148), np.nan); bound = np.full((B, 148), np.nan)
    P = np.zeros((B, 2)); Q = np.zeros((B, 2))
    d3 = det[:, None, None]; dd3 = dd[:, None, None]
    for left in (False, True):
        t0, dr0, di0, first = mlse_ref.half_tables(y[:, 0], w, h[:, 0], tsc, left)
        t1, dr1, di1, _ = mlse_ref.half_tables(yw, w, hw, tsc, left)
        n = (np.arange(0, 61)[None, :] + 4 + w[:, None]) if left else (np.arange(87, 148)[None, :] + w[:, None])      # the symbol a step reads
        c_re = (W_re[:, None] + oy_re[rows, n])[:, :, None]; c_im = (W_im[:, None] + oy_im[rows, n])[:, :, None]
        tab = d3 * t0 + t1
        fin = np.isfinite(tab)
        with np.errstate(invalid="ignore"):
            q0 = 4.0 * t0 + 8.0 * (np.abs(dr0) * Sr0 + np.abs(di0) * Si0)
            q1 = 4.0 * t1 + 2.0 * (np.abs(dr1) * c_re + np.abs(di1) * c_im)
            q3 = d3 * q0 + (dd3 + d3) * t0 + q1 + tab
        g = np.where(fin, tab, 0.0)
        q3 = np.where(fin, q3, 0.0)
        mm = mlse_ref.min_marginals(tab)                       # [B, 65, 2]
        ms = np.arange(0, 61) if left else np.arange(87, 148)
        D = mm[:, ms - first, 0] - mm[:, ms - first, 1]
        soft[:, ms] = 0.5 + D / (8.0 * E[:, None])
        P[:, int(left)] = g.max(axis=2).sum(axis=1); Q[:, int(left)] = q3.max(axis=2).sum(axis=1)
        bound[:, ms] = (SLACK * ((2.0 * Q[:, int(left)] + 124.0 * P[:, int(left)]) / (8.0 * E) + e / 2.0 + 2.0) * U)[:, None]
    return dict(soft=soft, bound=bound, E=E, e=e, det=det, P=P, Q=Q)


def sums64(y, w, h, tsc):
    """The residual sums in float64 on symbols y [B, 2, 148], windows w and taps h [B, 2, 5]: dict(sums [B, 4] (S00, S11, Xr, Xi),
    bound [B, 4])."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    h = np.ascontiguousarray(h, np.complex64).astype(np.complex128)
    w = np.asarray(w, np.int64)
    B = y.shape[0]
    a = 2.0 * mlse_ref.training_bits(tsc) - 1.0                # a[61 + j] = t[j]
    m = np.arange(65, 87)
    Z = sum(h[:, :, k][:, :, None] * a[m - 61 - k][None, None, :] for k in range(5))              # [B, 2, 22]
    n = m[None, :] + w[:, None]
    r = np.stack([y[np.arange(B)[:, None], 0, n], y[np.arange(B)[:, None], 1, n]], axis=1) - Z      # [B, 2, 22]
    rho_re = np.abs(r.real) + 4.0 * np.abs(h.real).sum(axis=2)[:, :, None]
    rho_im = np.abs(r.imag) + 4.0 * np.abs(h.imag).sum(axis=2)[:, :, None]
    r0, r1 = r[:, 0], r[:, 1]
    t00 = r0.real ** 2 + r0.imag ** 2; t11 = r1.real ** 2 + r1.imag ** 2
    X = r0 * np.conj(r1)
    tau00 = 2.0 * (np.abs(r0.real) * rho_re[:, 0] + np.abs(r0.imag) * rho_im[:, 0]) + 2.0 * t00
    tau11 = 2.0 * (np.abs(r1.real) * rho_re[:, 1] + np.abs(r1.imag) * rho_im[:, 1]) + 2.0 * t11
    tau_xr = (np.abs(r1.real) * rho_re[:, 0] + np.abs(r0.real) * rho_re[:, 1] + np.abs(r1.imag) * rho_im[:, 0] + np.abs(r0.imag) * rho_im[:, 1]
              + 2.0 * (np.abs(r0.real * r1.real) + np.abs(r0.imag * r1.imag)))
    tau_xi = (np.abs(r1.real) * rho_im[:, 0] + np.abs(r0.imag) * rho_re[:, 1] + np.abs(r1.imag) * rho_re[:, 0] + np.abs(r0.real) * rho_im[:, 1]
              + 2.0 * (np.abs(r0.imag * r1.real) + np.abs(r0.real * r1.imag)))
    terms = np.stack([t00, t11, X.real, X.imag], axis=1)       # [B, 4, 22]
    tau = np.stack([tau00, tau11, tau_xr, tau_xi], axis=1)
    return dict(sums=terms.sum(axis=2), bound=SLACK * (tau.sum(axis=2) + 21.0 * np.abs(terms).sum(axis=2)) * U)


def grade(soft, hard, y, w, h, cov, tsc):
    """mlse_ref.grade's three conditions (bad_soft, bad_clamp, bad_hard), `excluded` and `ratio` on soft [B, 148] float32 and hard
    [B, 148] against this reference on (y [B, 2, 148], w, h [B, 2, 5], cov [B, 4]).  The reference alone decides `excluded`."""
    return mlse_ref.graded(soft, hard, equalise64(y, w, h, cov, tsc), TRELLIS)


def check(soft, hard, y, w, h, cov, tsc, what):
    """Assert the three conditions; returns grade's dict."""
    return mlse_ref.checked(grade(soft, hard, y, w, h, cov, tsc), soft, hard, what)


def check_sums(sums, y, w, h, tsc, what):
    """Assert |S32 - S64| <= bound for the four residual sums [B, 4]; returns the worst fraction of the bound."""
    r = sums64(y, w, h, tsc)
    err = np.abs(np.asarray(sums, np.float32).astype(np.float64) - r["sums"])
    assert np.all(err <= r["bound"]), "%s: a residual sum is off by %.3g of its bound" % (what, float((err / r["bound"]).max()))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(r["bound"] > 0, err / r["bound"], 0.0)))
