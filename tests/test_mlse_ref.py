"""The sequence equaliser's float32 model (tests/mlse_model.py) graded against the float64 reference (tests/mlse_ref.py): the
reference's min-marginal routine against the enumeration of every assignment; the census of the family
(tests/mlse_ref_family.py); the model's soft and hard bits within the reference's a-priori bound on every family burst and on
mlse_family.mixed_batch; the estimator; and six one-token mutants of the model, each of which the comparison must catch.  No GPU:
tests/test_gpu_mlse_ref.py holds the kernel to the same reference."""
import numpy as np
import pytest

import mlse_family
import mlse_model as mm
import mlse_ref as ref
import mlse_ref_family as fam
import synth
from mlse_variant import variant

MIXED_SNR = [np.nan, 12.0, 15.0, 15.0, np.nan, 8.0]           # mlse_family.mixed_batch's kinds, burst b is kind b % 6


# ---- the min-marginal routine ----
def enumerate_min_marginals(tab):
    """Every one of the 2^(L+4) assignments of a [L, 32] chain, summed factor by factor: [L + 4, 2]."""
    L = tab.shape[0]
    n = L + 4
    bits = (np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1
    total = np.zeros(1 << n)
    for l in range(L):
        total = total + tab[l, (bits[:, l:l + 5] << np.arange(5)[None, :]).sum(axis=1)]
    out = np.empty((n, 2))
    for v in range(n):
        for b in (0, 1):
            out[v, b] = total[bits[:, v] == b].min()
    return out


def chain_cases():
    rng = np.random.default_rng(2024)
    cases = []
    for i in range(12):
        tab = rng.uniform(0.0, 4.0, (8, 32)) ** 2
        if i % 3 == 1:                                        # forbidden entries at random, a quarter of them in one case
            tab[rng.uniform(size=tab.shape) < (0.25 if i == 4 else 0.08)] = np.inf
        if i % 3 == 2 or i == 7:                              # pinned variables: both ends as the two halves have them, and one inside
            for v, b in ((0, 1), (1, 0), (2, 0), (3, 1), (9, 0), (10, 0), (11, 0)) if i % 2 else ((5, 1), (11, 0)):
                ref.pin(tab, v, b)
        cases.append(tab)
    contradiction = rng.uniform(0.0, 4.0, (8, 32))
    ref.pin(contradiction, 4, 0)
    contradiction[4, (np.arange(32) & 1) == 0] = np.inf     # variable 4 must be 0 and must not be 0: nothing is allowed
    cases.append(contradiction)
    return cases


def test_min_marginals_equal_the_enumeration():
    """Random [8, 32] tables (12 variables, 4096 assignments), plain, with +inf entries and with pinned variables: the infinities are
    in identical places and the finite values agree to 1e-13 relative (the order of summation differs).  A stack of tables in one
    call gives what the tables give one by one."""
    cases = chain_cases()
    stacked = ref.min_marginals(np.stack(cases))
    n_inf = 0
    for i, tab in enumerate(cases):
        want = enumerate_min_marginals(tab)
        got = ref.min_marginals(tab)
        assert got.shape == (12, 2)
        assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any(), i
        fin = np.isfinite(want)
        assert np.all(np.abs(got[fin] - want[fin]) <= 1e-13 * np.abs(want[fin])), i
        assert np.array_equal(stacked[i], got), i
        n_inf += int(np.isinf(want).sum())
    assert n_inf >= 20 and np.isinf(ref.min_marginals(cases[-1])).all()


# ---- the family ----
def test_census():
    """The conditions the family is built to meet, on the reference's quantities (the float64 estimator, the symbols)."""
    batches = fam.family()
    assert sum(len(f["name"]) for f in batches) <= 400
    lone_at = {1: set(), 2: set(), 4: set()}
    snrs, groups = set(), set()
    for f in batches:
        y = f["want"]["y"]
        assert np.all(f["want"]["win"] <= 0), "a family burst is not equalised"
        e = ref.estimate64(y, f["tsc"])
        w64 = -np.argmax(e["E"], axis=1)
        E64 = e["E"].max(axis=1)
        assert np.all((E64 > 2.0 ** -50) & (E64 < 2.0 ** 50))
        big = np.maximum(np.abs(y.real), np.abs(y.imag))
        assert big.max() < 2.0 ** 29                          # nowhere near the 2^30 fallback
        assert np.all((big == 0) | (big > 2.0 ** -60))        # a square of it is a normal float32
        sel = f["group"] == "windows"
        if sel.any():
            assert set(w64[sel].tolist()) == {0, -1, -2, -3, -4}, (f["sps"], f["tsc"], w64[sel])
        for b in np.flatnonzero(f["group"] == "lone"):
            h = e["c"][b, w64[b] + 4:w64[b] + 9]
            k = int(np.abs(h).argmax())
            assert np.abs(h[k]) ** 2 > 0.9 * E64[b]
            lone_at[f["sps"]].add(k)
            if f["shift"][b] == fam.LONE_AT_H0:
                assert k == 0
            if f["shift"][b] == fam.LONE_AT_H4:
                assert k == 4
        sel = f["group"] == "scale"
        if sel.any():
            assert sorted(set(f["k"][sel].tolist())) == sorted(fam.SCALES)
            for k in fam.SCALES:                              # the multiplier is exact: E scales by 2^-2k against the k = 0 twin's order of magnitude
                ratio = E64[sel & (f["k"] == k)].mean() / E64[sel & (f["k"] == 0)].mean() * 4.0 ** k
                assert 0.25 < ratio < 4.0, (k, ratio)
        assert (f["off"] % 2 == 1).any() and (f["off"] % 2 == 0).any()
        snrs |= set(("none" if np.isnan(v) else v) for v in f["snr"][f["group"] == "noise"])
        groups |= set(f["group"].tolist())
    for sps in (1, 2, 4):
        lengths = np.concatenate([f["length"] for f in batches if f["sps"] == sps])
        assert (lengths == 157 * sps).any() and (lengths == 156 * sps).any()
    assert sorted(set(f["tsc"] for f in batches if f["sps"] == 1 and (f["group"] == "windows").any())) == list(range(8))
    assert all(lone_at[s] == {0, 1, 2, 3, 4} for s in (1, 2, 4)), lone_at
    assert snrs == {"none", 15.0, 6.0, 0.0}
    assert groups == {"windows", "lone", "channels", "noise", "scale"}
    assert {g for f in batches if f["sps"] > 1 for g in f["group"]} == {"windows", "lone", "channels"}


def sources(which):
    """(batch, snr [B], group [B], named [B, 148] or None) of the family or of mixed_batch at one rate."""
    if which == "family":
        return [(f, f["snr"], f["group"], fam.named_edges(f)) for f in fam.family()]
    f = mlse_family.mixed_batch(which, 2, 67, 4100 + which)
    return [(f, np.array([MIXED_SNR[b % 6] for b in range(67)]), np.array(["mixed sps %d" % which] * 67), None)]


@pytest.mark.parametrize("which", ["family", 1, 2, 4])
def test_model_within_the_bound(which):
    """On every trellis position of every burst: |model soft - clamp(soft64)| <= bound; the model's soft bit is exactly 0 or 1 where
    soft64 is outside [0, 1] by more than the bound; hard bits equal wherever |soft64 - 0.5| > bound.  The positions the reference
    keeps out of the hard-bit comparison are at most 0.5 % of the payload positions of any noise level; the named edge symbols of the
    lone-tap members are held to |soft - 0.5| <= bound instead where the reference finds them inside the margin.  Measured on the
    CPU: the worst error is 0.5 % of the bound (printed per group)."""
    tally = ref.Tally(mlse_family.PAYLOAD)
    for f, snr, group, named in sources(which):
        wt = f["want"]
        eq = wt["win"] <= 0
        assert eq.sum() >= len(eq) - 2
        g = ref.check(wt["soft"][eq], wt["hard"][eq], wt["y"][eq], wt["win"][eq], wt["chan"][eq], f["tsc"],
                      "model, %s sps %d tsc %d" % (which, f["sps"], f["tsc"]), named=None if named is None else named[eq])
        tally.add(g, snr[eq], group[eq], None if named is None else named[eq])
    tally.report("model (CPU), %s" % which)
    tally.assert_cap("model, %s" % which)


def test_exact_lone_tap():
    """Synthetic symbols y = h0 a + clipped noise with exactly one non-zero tap, at each of h[0]..h[4] in turn, w = -2.  The
    reference is the demodulator's (Re(y / h0) + 1) / 2 on every observed position (M_0 - M_1 = 4 Re(y conj(h0)) once all other
    terms are shared), to 1e-9; with the tap on h[0] the left half never reads the sample that carries a[3], with it on h[4] the
    right half never reads a[144]'s: soft64 is exactly 0.5 there and the model within the bound of it; the model is within the
    bound everywhere."""
    rng = np.random.default_rng(78)
    tsc, n, w0 = 6, 8, -2
    bits = synth.normal_bits(rng, n, tsc)
    h0 = np.complex64(0.8 * np.exp(2j * np.pi * rng.uniform()))
    E = np.full(n, np.float32(h0.real) * np.float32(h0.real) + np.float32(h0.imag) * np.float32(h0.imag), np.float32)
    for k in range(5):
        a = np.zeros((n, 148 + 16)); a[:, 8:156] = 2.0 * bits - 1.0
        lo = 8 - w0 - k                                       # y[m] = h0 a[m - w0 - k]
        noise = np.clip(0.05 * rng.standard_normal((2, n, 148)), -0.15, 0.15)
        y = (np.complex128(h0) * (a[:, lo:lo + 148] + noise[0] + 1j * noise[1])).astype(np.complex64)
        h = np.zeros((n, 5), np.complex64); h[:, k] = h0
        w = np.full(n, w0, np.int32)
        soft = mm.trellis(y, tsc, w, h, E)
        g = ref.check(soft, soft > 0.5, y, w, h, tsc, "lone tap on h[%d]" % k)
        s64 = g["ref"]["soft"]
        observed = np.ones(148, bool); observed[61:87] = False; observed[[0, 1, 2, 145, 146, 147]] = False
        if k == 0:
            observed[3] = False
            assert np.all(s64[:, 3] == 0.5) and np.all(np.abs(soft[:, 3] - 0.5) <= g["ref"]["bound"][:, 3])
        if k == 4:
            observed[144] = False
            assert np.all(s64[:, 144] == 0.5) and np.all(np.abs(soft[:, 144] - 0.5) <= g["ref"]["bound"][:, 144])
        ms = np.flatnonzero(observed)
        dem = (np.real(y.astype(np.complex128)[:, ms + w0 + k] / np.complex128(h0)) + 1.0) / 2.0
        assert np.abs(s64[:, ms] - dem).max() < 1e-9, k


def test_estimator_within_its_bounds():
    """On every family burst and on mixed_batch (noisy multipath, all rates): |c - c64| <= 16 u Ymax per component, and the window the
    model takes has E64[w] >= max E64 - tolE (mlse_ref's docstring derives both); the taps it hands on are c[w..w+4]."""
    worst_c = worst_E = 0.0
    n = 0
    for which in ("family", 1, 2, 4):
        for f, _, _, _ in sources(which):
            wt = f["want"]
            eq = wt["win"] <= 0
            y, win = wt["y"][eq], wt["win"][eq]
            c, w, h, E = mm.estimate(y, mm.tsc_symbols(f["tsc"]))
            assert np.array_equal(w, win) and wt["chan"][eq].tobytes() == h.tobytes()
            e = ref.estimate64(y, f["tsc"])
            err = np.maximum(np.abs(c.real - e["c"].real), np.abs(c.imag - e["c"].imag)).max(axis=1)
            assert np.all(err <= e["tol_c"]), (which, f["sps"], f["tsc"])
            gap = e["E"].max(axis=1) - e["E"][np.arange(len(w)), -w]
            assert np.all(gap <= e["tol_E"]), (which, f["sps"], f["tsc"])
            rows = np.arange(len(w))[:, None]
            assert np.array_equal(h, c[rows, (w + 4)[:, None] + np.arange(5)[None, :]])
            worst_c = max(worst_c, float((err / e["tol_c"]).max())); worst_E = max(worst_E, float((gap / e["tol_E"]).max()))
            n += len(w)
    print("estimator (CPU), %d bursts: worst |c - c64| / (16 u Ymax) = %.3f, worst window gap / tolE = %.3g" % (n, worst_c, worst_E))


# ---- mutants: the comparison can fail ----
MUTANTS = {   # name: (the token -- in the model's text, or in that of the shared pieces it calls --, its replacement)
    "right start state bit-reversed": ("bit[25] | (bit[24] << 1) | (bit[23] << 2) | (bit[22] << 3)",
                                       "bit[22] | (bit[23] << 1) | (bit[24] << 2) | (bit[25] << 3)"),
    "tail from step 59": ("i >= steps - 3:", "i >= steps - 2:"),
    "left half's taps not reversed": ("_half(yr, yi, w, hr[:, ::-1], hi[:, ::-1], start_l, True)", "_half(yr, yi, w, hr, hi, start_l, True)"),
    "left sample index m + 3 + w": ("(first - i + 4 + sign_w * w)", "(first - i + 3 + sign_w * w)"),
    "window energies over four taps": ("(((p[:, k] + p[:, k + 1]) + p[:, k + 2]) + p[:, k + 3]) + p[:, k + 4]",
                                       "((p[:, k] + p[:, k + 1]) + p[:, k + 2]) + p[:, k + 3]"),
    "8 E replaced by 4 E": ("F(8.0) * E", "F(4.0) * E"),
}


def worst_ratio(model, batches):
    """The largest |soft - clamp(soft64)| / bound of `model` on the batches, graded exactly as the model itself is: its soft bits
    against the reference on its own window and taps."""
    worst = 0.0
    for f in batches:
        soft, win, h = model.equalise(f["want"]["y"], f["tsc"])
        assert np.all(win <= 0)
        worst = max(worst, float(ref.grade(soft, soft > 0.5, f["want"]["y"], win, h, f["tsc"])["ratio"].max()))
    return worst


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_is_caught(name):
    """Each mutant exceeds the bound on at least one family burst (the unmutated copy, built the same way, stays inside)."""
    batches = fam.batches(1)
    if name == sorted(MUTANTS)[0]:
        assert worst_ratio(variant(mm), batches) <= 1.0
    worst = worst_ratio(variant(mm, MUTANTS[name]), batches)
    print("mutant %-32s worst |soft - clamp(soft64)| / bound = %.3g" % (name, worst))
    assert worst > 1.0
