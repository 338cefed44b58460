"""The float64 reference of the sequence equaliser (trxsig_mlse_batch): step 3 of the header's comment read as a statement about
SEQUENCES, with no trellis vocabulary -- no states, no predecessors, no alpha or beta.  tests/mlse_model.py and the kernel are
graded against it (tests/test_mlse_ref.py, tests/test_gpu_mlse_ref.py); nothing here is imported from, or shared with, either.

The operation.  With the burst model y[n] = sum_k h[k] a[n - w - k], a[n] = +-1, the soft bit of symbol m is
    soft64[m] = 0.5 + (M_0 - M_1) / (8 E64),       E64 = sum_k |h[k]|^2,
where M_b is the minimum, over every symbol sequence that agrees with the known symbols and has bit m = b, of the summed squared
error.  The two halves, in absolute symbol indices (t[j] = a[61 + j] is the training sequence):
    right   variables a[83..147]; one term |y[m + w] - sum_k h[k] a[m - k]|^2 per m = 87..147;
            a[83..86] = training bits 22..25, a[145..147] = -1;
    left    variables a[0..64]; one term |y[m + 4 + w] - sum_k h[k] a[m + 4 - k]|^2 per m = 0..60;
            a[61..64] = training bits 0..3, a[0..2] = -1.
Every term touches five consecutive symbols, so each half is a chain of 65 binary variables with 61 factors of 32 entries, and
M_b is a min-marginal of that chain: min_marginals() computes them exactly (the test proves it against the enumeration of all
assignments on a short chain).  Inputs are the float32 symbols y[148], the window w and the five float32 taps, widened to float64.

The bound on |soft32 - clamp(soft64)| (bound_terms), u = 2^-24, to first order in u; float64's own rounding (2^-53 where float32
has 2^-24) and the second-order terms are covered by the factor 1.001.  Per burst and per half, from the reference's quantities
only.  Write Sr = sum_k |Re h[k]|, Si = sum_k |Im h[k]|.
  * One branch metric.  Z is four float32 additions of +-h[k]: each part is off by <= 4 u Sr (4 u Si).  dr = y.re - Z.re rounds
    once more: |dr32 - dr| <= u |dr| + 4 u Sr.  The square carries twice that times |dr| plus its own rounding, 3 u dr^2 +
    8 u |dr| Sr; the same for di; the sum of the two rounds once more.  In all
        |g32 - g| <= u (4 g + 8 (|dr| Sr + |di| Si)) =: u q(g).
    (Not "a few u relative": near a good fit g is small while the rounding of Z is not.)
  * Sums.  Let G_i be the largest finite branch metric of step i and P = sum_i G_i: P bounds every finite path metric, partial ones
    too.  Let Q = sum_i max_x q over the finite branches of step i.  A minimum of perturbed numbers is off by no more than the
    largest perturbation, and +inf stays +inf (a known symbol, the start state), so by induction along the steps a forward metric
    after step i is off by <= u sum_{j <= i} q_j + (i + 1) u P (one rounded addition of a value <= P per step), a backward one by
    <= u sum_{j > i} q_j + (60 - i) u P, and T = alpha + beta rounds once more: |T32 - T| <= u (Q + 62 P), and so is each M_b.
  * D = M_0 - M_1 rounds once: |D32 - D| <= 2 u (Q + 62 P) + u |D|.
  * The quotient.  E32 is five products-and-sums p[d] (2 u relative each) and four additions of positive numbers: E32 = E64 (1 + e),
    |e| <= 6 u.  8 E32 is exact, the division rounds once: |D32 / (8 E32) - D / (8 E64)| <= 2 u (Q + 62 P) / (8 E64) + 8 u |D / (8 E64)|.
    The last addition rounds u |soft|.  Where soft64 lies in [0, 1] the two last terms are <= 4 u + u.  Where it lies outside by t,
    the terms grow by 9 u t while the distance to the clamp grows by t: the clamp is hit exactly once t exceeds the bound; the
    clamp is 1-Lipschitz, so the same bound holds against clamp(soft64).
        bound = 1.001 * ((2 Q + 124 P) / (8 E64) + 5) * u
  Q is at most (4 + 8 sqrt 2) P on untailed steps (Z and -Z are both expected values, so G_i >= (Sr^2 + Si^2) / 2), which gives a
  closed form of about (155 P / (8 E64) + 5) u; the code uses Q itself.  Nothing here was fitted to an observed error.

The estimator.  c64[d] = (1/16) sum_i t[5 + i] y[66 + i + d] and the five window energies in float64.  With Ymax the largest
component magnitude among y[62..85] (what the sums read): the float32 inputs are exact, the first addition (to 0) is exact, each of
the other 15 rounds a partial sum of magnitude <= 16 Ymax, the product with 1/16 is exact: |c32 - c64| <= 15 u Ymax <= 16 u Ymax per
component (tests/test_mlse_model.py's derivation).  With e = 16 u Ymax: |p32 - p64| <= 2 (|c.re| + |c.im|) e + 2 e^2 + 2 u p, and the
four additions of a window add 4 u E: |E32_w - E64_w| <= tau_w = sum_{d in w} (2 (|c.re| + |c.im|) e + 2 e^2) + 6 u E64_w.  The scan
takes a largest E32, so the window it takes has E64[w] >= max E64 - 2 max_w tau_w =: tolE (times 1.001 as above).
"""
import numpy as np

import synth

U = 2.0 ** -24                                                # float32 unit roundoff
SLACK = 1.001                                                 # second-order terms and float64's own rounding
TRELLIS = np.r_[0:61, 87:148]                                 # the positions the two chains decide
_X = np.arange(32)


def min_marginals(tab):
    """Exact min-marginals of a chain of L + 4 binary variables with one factor per five consecutive variables.  tab [..., L, 32]
    float64: tab[l, x] is the cost of factor l when variable l + j has the value bit j of x (+inf forbids).  Returns [..., L + 4, 2]:
    for every variable and both values the minimum total over all assignments (+inf if none is allowed)."""
    tab = np.asarray(tab, np.float64)
    lead, L = tab.shape[:-2], tab.shape[-2]
    low, high = _X & 15, _X >> 1                              # x's variables l..l+3 and l+1..l+4, as 4-bit words
    before = np.zeros(lead + (L, 16)); after = np.zeros(lead + (L, 16))
    f = np.zeros(lead + (16,))
    for l in range(L):                                        # before[l][v]: the cheapest way through factors < l ending in l..l+3 = v
        before[..., l, :] = f
        t = f[..., low] + tab[..., l, :]
        f = np.minimum(t[..., 0::2], t[..., 1::2])            # variable l drops out; what is left is x >> 1
    b = np.zeros(lead + (16,))
    for l in range(L - 1, -1, -1):                            # after[l][v]: the cheapest way through factors > l starting from l+1..l+4 = v
        after[..., l, :] = b
        t = tab[..., l, :] + b[..., high]
        b = np.minimum(t[..., :16], t[..., 16:])              # variable l+4 drops out; what is left is x & 15
    total = before[..., low] + tab + after[..., high]         # [..., L, 32]: the cheapest assignment with factor l's five variables = x
    out = np.empty(lead + (L + 4, 2))
    for v in range(L + 4):
        l = min(v, L - 1)
        bit = (_X >> (v - l)) & 1
        out[..., v, 0] = total[..., l, bit == 0].min(axis=-1)
        out[..., v, 1] = total[..., l, bit == 1].min(axis=-1)
    return out


def pin(tab, var, value):
    """Forbid, in place, every entry of tab [..., L, 32] in which chain variable `var` is not `value` (0 or 1)."""
    L = tab.shape[-2]
    for l in range(max(0, var - 4), min(L - 1, var) + 1):
        tab[..., l, ((_X >> (var - l)) & 1) != value] = np.inf


def training_bits(tsc):
    return np.array([int(ch) for ch in synth.TRAINING_SEQUENCE[tsc]], np.int64)


def chain_tables(y, w, h, n, first, known):
    """The factor tables of one chain, [B, L, 32], with the known symbols pinned, and (dr, di) [B, L, 32] for the bound: (tab, dr,
    di).  Chain variable v is a[first + v]; factor l covers a[first + l .. first + l + 4], the newest of them against tap h[0], and
    reads y[n[l] + w]; known {m: bit} pins a[m].  Every equaliser's reference builds its tables here."""
    y = np.asarray(y, np.complex128); h = np.asarray(h, np.complex128); w = np.asarray(w, np.int64)
    B = y.shape[0]
    a = 2.0 * ((_X[:, None] >> np.arange(5)[None, :]) & 1) - 1.0            # a[x, j]: the value of the factor's j-th symbol
    Z = (a[None, :, :] * h[:, None, ::-1]).sum(axis=2)                      # sum_k h[k] a[newest - k], newest = j = 4
    d = y[np.arange(B)[:, None], np.asarray(n)[None, :] + w[:, None]][:, :, None] - Z[:, None, :]
    tab = d.real ** 2 + d.imag ** 2
    for m, v in known.items():
        pin(tab, m - first, v)
    return tab, d.real, d.imag


def half_tables(y, w, h, tsc, left):
    """chain_tables of one half of a normal burst, [B, 61, 32], and the chain's first symbol: (tab, dr, di, first)."""
    t = training_bits(tsc)
    if left:                                                  # m = 0..60 reads y[m + 4 + w]; factor m covers a[m..m+4]
        first, n, known = 0, np.arange(0, 61) + 4, {61 + j: int(t[j]) for j in range(4)}
        known.update({0: 0, 1: 0, 2: 0})
    else:                                                     # m = 87..147 reads y[m + w]; factor m - 87 covers a[m-4..m]
        first, n, known = 83, np.arange(87, 148), {61 + j: int(t[j]) for j in range(22, 26)}
        known.update({145: 0, 146: 0, 147: 0})
    return chain_tables(y, w, h, n, first, known) + (first,)


def bound_terms(tab, dr, di, h):
    """(P, Q) [B] of the module docstring for one half."""
    h = np.asarray(h, np.complex128)
    Sr = np.abs(h.real).sum(axis=1)[:, None, None]; Si = np.abs(h.imag).sum(axis=1)[:, None, None]
    fin = np.isfinite(tab)
    g = np.where(fin, tab, 0.0)
    q = np.where(fin, 4.0 * tab + 8.0 * (np.abs(dr) * Sr + np.abs(di) * Si), 0.0)
    return g.max(axis=2).sum(axis=1), q.max(axis=2).sum(axis=1)


def equalise64(y, w, h, tsc):
    """The reference on symbols y [B, 148] (complex64), windows w [B] and taps h [B, 5] (complex64): dict(soft [B, 148] float64,
    unclamped, NaN on 61..86; bound [B, 148], the a-priori bound on |soft32 - clamp(soft64)| (per half; NaN on 61..86); E [B];
    P, Q [B, 2], right and left)."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    h = np.ascontiguousarray(h, np.complex64).astype(np.complex128)
    w = np.asarray(w, np.int64)
    assert y.ndim == 2 and y.shape[1] == 148 and h.shape == (y.shape[0], 5) and np.all((w >= -4) & (w <= 0))
    B = y.shape[0]
    E = (h.real ** 2 + h.imag ** 2).sum(axis=1)
    soft = np.full((B, 148), np.nan); bound = np.full((B, 148), np.nan)
    P = np.zeros((B, 2)); Q = np.zeros((B, 2))
    for left in (False, True):
        tab, dr, di, first = half_tables(y, w, h, tsc, left)
        mm = min_marginals(tab)                               # [B, 65, 2]
        ms = np.arange(0, 61) if left else np.arange(87, 148)
        D = mm[:, ms - first, 0] - mm[:, ms - first, 1]       # minmarg[a[m] = -1] - minmarg[a[m] = +1]
        soft[:, ms] = 0.5 + D / (8.0 * E[:, None])
        P[:, int(left)], Q[:, int(left)] = bound_terms(tab, dr, di, h)
        bound[:, ms] = (SLACK * ((2.0 * Q[:, int(left)] + 124.0 * P[:, int(left)]) / (8.0 * E) + 5.0) * U)[:, None]
    return dict(soft=soft, bound=bound, E=E, P=P, Q=Q)


def estimate64(y, tsc):
    """The estimator in float64 on symbols y [B, 148]: dict(c [B, 9] for d = -4..4; E [B, 5], E[:, q] the energy of window w = -q;
    tol_c [B], the bound on |c32 - c64| per component; tol_E [B], how far below the largest the chosen window's E64 may lie)."""
    y = np.ascontiguousarray(y, np.complex64).astype(np.complex128)
    t = 2.0 * training_bits(tsc) - 1.0
    c = np.stack([(t[5:21][None, :] * y[:, 66 + d:82 + d]).sum(axis=1) / 16.0 for d in range(-4, 5)], axis=1)
    p = c.real ** 2 + c.imag ** 2
    E = np.stack([p[:, 4 - q:9 - q].sum(axis=1) for q in range(5)], axis=1)
    ymax = np.maximum(np.abs(y[:, 62:86].real), np.abs(y[:, 62:86].imag)).max(axis=1)
    e = 16.0 * U * ymax
    per = 2.0 * (np.abs(c.real) + np.abs(c.imag)) * e[:, None] + 2.0 * (e ** 2)[:, None]
    tau = np.stack([per[:, 4 - q:9 - q].sum(axis=1) for q in range(5)], axis=1) + 6.0 * U * E
    return dict(c=c, E=E, tol_c=e, tol_E=SLACK * 2.0 * tau.max(axis=1))


def graded(soft, hard, r, positions):
    """The three conditions on soft [B, 148] float32 and hard [B, 148] (0/1) against a reference r (an equalise64's dict) on the
    trellis positions it decides:
      bad_soft  [B, 148]  |soft - clamp(soft64)| > bound                                  (trellis positions)
      bad_clamp [B, 148]  soft64 outside [0, 1] by more than the bound and soft not exactly 0 / 1
      bad_hard  [B, 148]  |soft64 - 0.5| > bound and the hard bit is not soft64 > 0.5
      excluded  [B, 148]  trellis positions the reference keeps out of the hard-bit comparison (|soft64 - 0.5| <= bound)
      ratio     [B, 148]  |soft - clamp(soft64)| / bound (0 off the trellis)
    The reference alone decides `excluded`.  Every equaliser's grade() is this on its own reference and positions."""
    s64, bd = r["soft"], r["bound"]
    on = np.zeros(148, bool); on[positions] = True
    s32 = np.asarray(soft, np.float32)[:, :148].astype(np.float64)
    hb = np.asarray(hard)[:, :148] != 0
    with np.errstate(invalid="ignore"):
        err = np.abs(s32 - np.clip(s64, 0.0, 1.0))
        bad_soft = on[None, :] & ~(err <= bd)                 # (a NaN soft bit is bad)
        low, high = s64 < -bd, s64 > 1.0 + bd
        bad_clamp = on[None, :] & ((low & (s32 != 0.0)) | (high & (s32 != 1.0)))
        decided = on[None, :] & (np.abs(s64 - 0.5) > bd)
        bad_hard = decided & (hb != (s64 > 0.5))
        ratio = np.where(on[None, :], err / bd, 0.0)
    return dict(bad_soft=bad_soft, bad_clamp=bad_clamp, bad_hard=bad_hard, excluded=on[None, :] & ~decided, ratio=ratio, ref=r)


def grade(soft, hard, y, w, h, tsc, ref=None):
    """graded() against the reference on (y, w, h), or against a given one."""
    return graded(soft, hard, ref or equalise64(y, w, h, tsc), TRELLIS)


def checked(g, soft, hard, what):
    """Assert the three conditions of a grade()'s dict g; returns g."""
    r = g["ref"]
    for key, text in (("bad_soft", "|soft - clamp(soft64)| > bound"), ("bad_clamp", "soft64 beyond the clamp by more than the bound, soft not clamped"),
                      ("bad_hard", "hard bit differs outside the margin")):
        if g[key].any():
            b, m = np.argwhere(g[key])[0]
            raise AssertionError("%s: %s at %d positions; first: burst %d symbol %d: soft %.9g hard %d, soft64 %.12g, bound %.3g"
                                 % (what, text, g[key].sum(), b, m, np.asarray(soft)[b, m], np.asarray(hard)[b, m], r["soft"][b, m], r["bound"][b, m]))
    return g


def check(soft, hard, y, w, h, tsc, what, named=None):
    """Assert the three conditions (grade) and, on the named barely-observed positions the reference keeps out of the hard-bit
    comparison, |soft - 0.5| <= bound.  Returns grade's dict."""
    g = checked(grade(soft, hard, y, w, h, tsc), soft, hard, what)
    r = g["ref"]
    if named is not None:
        at = named & g["excluded"]
        dev = np.abs(np.asarray(soft, np.float32)[:, :148].astype(np.float64) - 0.5)
        assert np.all(dev[at] <= r["bound"][at]), "%s: a named edge symbol is further than the bound from 0.5" % what
    return g


class Tally:
    """Counts, per noise level, the payload positions the reference keeps out of the hard-bit comparison (the named edge symbols
    apart), and keeps the worst error / bound ratio per group."""
    CAP = 0.005

    def __init__(self, payload):
        self.payload = np.asarray(payload)
        self.excluded, self.positions, self.worst = {}, {}, {}

    def add(self, g, snr, group, named=None):
        ex = g["excluded"] if named is None else g["excluded"] & ~named
        for b in range(len(snr)):
            key = "no noise" if np.isnan(snr[b]) else "%g dB" % snr[b]
            self.excluded[key] = self.excluded.get(key, 0) + int(ex[b, self.payload].sum())
            self.positions[key] = self.positions.get(key, 0) + len(self.payload)
            self.worst[str(group[b])] = max(self.worst.get(str(group[b]), 0.0), float(g["ratio"][b].max()))

    def report(self, what):
        for k in sorted(self.worst):
            print("%s: %-10s worst |soft - clamp(soft64)| / bound = %.4f" % (what, k, self.worst[k]))
        for k in sorted(self.excluded):
            print("%s: %-10s %d of %d payload positions inside the margin" % (what, k, self.excluded[k], self.positions[k]))

    def assert_cap(self, what):
        for k in self.excluded:
            assert self.excluded[k] <= self.CAP * self.positions[k], "%s, %s: %d of %d payload positions excluded from the hard-bit comparison" \
                % (what, k, self.excluded[k], self.positions[k])
