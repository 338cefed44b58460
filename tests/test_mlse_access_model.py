"""The access-burst sequence equaliser's float32 model (tests/mlse_access_model.py): its least-squares table from Python integers,
the model graded against the float64 reference (tests/mlse_access_ref.py) within the bounds derived there, four one-change mutants
that the grading must catch, and what the equaliser buys over demodulateBurst on seeded multipath families.  No GPU:
tests/test_gpu_mlse_access.py holds the kernel to the model word for word, tests/test_gpu_mlse_access_ref.py to the reference."""
import numpy as np
import pytest

import fecbind
import mlse_access_family as family
import mlse_access_model as model
import mlse_access_ref as ref
import mlse_family
from mlse_ref import U

B_ALL = 37


def batch(sps):
    return family.mixed_batch(sps, B_ALL, 5100 + sps)          # (shared with the GPU tests: computed once per process)


# ---- the table ----
def test_table_from_integers():
    """G = A^T A is 41 on the diagonal and at most 5 off it; N = adj(G) A^T and det(G) are exact integers below 2^53, so the double
    division and the float32 rounding are each ONE correct rounding; |P32| < 0.04; P32 A is the identity to within the roundings of
    P32's entries: entry (d, e) of P32 A - I is sum_j (P32 - P)[d][j] A[j][e] with |A| = 1 and |P32 - P| <= 2^-25 |P| (2^-24 is the
    spacing, half of it the rounding; the double division's 2^-53 is covered by the factor 1.001), so it is at most
    1.001 * 2^-25 * sum_j |P[d][j]| over the 41 terms -- evaluated here in exact rational arithmetic."""
    from fractions import Fraction
    A = model.design_matrix()
    G = [[sum(A[n][i] * A[n][j] for n in range(41)) for j in range(9)] for i in range(9)]
    assert all(G[i][i] == 41 for i in range(9)) and max(abs(G[i][j]) for i in range(9) for j in range(9) if i != j) <= 5
    N, det = model.pinv_integers()
    assert 0 < det < 2 ** 53 and all(abs(v) < 2 ** 53 for row in N for v in row)
    for i in range(9):                                        # N / det IS the pseudo-inverse: (N A) = det * I, exactly
        for e in range(9):
            assert sum(N[i][n] * A[n][e] for n in range(41)) == (det if i == e else 0)
    P32 = model.pinv_table()
    assert P32.shape == (9, 41) and P32.dtype == np.float32 and np.abs(P32).max() < 0.04
    for i in range(9):
        for n in range(41):
            assert P32[i, n] == np.float32(np.float64(N[i][n]) / np.float64(det))
    worst = 0.0
    for d in range(9):
        bound = Fraction(1001, 1000) * Fraction(1, 2 ** 25) * sum(abs(Fraction(N[d][j], det)) for j in range(41))
        for e in range(9):
            dev = abs(sum(Fraction(float(P32[d, j])) * A[j][e] for j in range(41)) - int(d == e))
            assert dev <= bound, (d, e, float(dev), float(bound))
            worst = max(worst, float(dev / bound))
    gain = (P32.astype(np.float64) ** 2).sum(axis=1)          # the estimator's noise gain per tap
    assert 0.0248 <= gain.min() and gain.max() <= 0.0258, gain
    print("P32 A - I: worst entry at %.3f of its bound; noise gain %.4f to %.4f per tap" % (worst, gain.min(), gain.max()))


def test_start_state_and_head():
    assert model.START == 8 and len(model.HEAD) == 49         # a[48], a[47], a[46], a[45] = bits 0, 0, 0, 1


# ---- the model against the float64 statement ----
@pytest.mark.parametrize("sps", [1, 2, 4])
def test_model_within_the_bound(sps):
    """On positions 49..87 of every burst of the mixed batch: |model soft - clamp(soft64)| <= bound; exactly 0 or 1 where soft64 is
    outside [0, 1] by more than the bound (the three tail bits among them: soft64 = -inf, the model exactly 0); hard bits equal
    wherever |soft64 - 0.5| > bound, and the positions inside that margin are at most 0.5 % of the payload."""
    f = batch(sps)
    wt = f["want"]
    eq = wt["win"] <= 0
    assert eq.sum() >= B_ALL - 2
    g = ref.check(wt["soft"][eq], wt["hard"][eq], wt["y"][eq], wt["win"][eq], wt["chan"][eq], "model, sps %d" % sps)
    assert np.all(wt["soft"][eq][:, 85:88] == 0.0) and np.all(np.isneginf(g["ref"]["soft"][:, 85:88]))
    ex = int(g["excluded"][:, family.PAYLOAD].sum())
    print("model (CPU), sps %d: worst |soft - clamp(soft64)| / bound = %.4f (bound %.2e to %.2e); %d of %d payload positions inside the margin"
          % (sps, g["ratio"].max(), np.nanmin(g["ref"]["bound"]), np.nanmax(g["ref"]["bound"]), ex, eq.sum() * 36))
    assert ex <= 0.005 * eq.sum() * 36


def estimator_ratios(f, P32=None):
    """(worst |c32 - c64| / tol_c, worst window gap / tol_E) of the model's estimator (with table P32) on batch f."""
    wt = f["want"]
    eq = wt["win"] <= 0
    y = wt["y"][eq]
    c, w, h, E = model.estimate(y, P32)
    e = ref.estimate64(y, model.pinv_table())
    err = np.maximum(np.abs(c.real - e["c"].real), np.abs(c.imag - e["c"].imag))
    gap = e["E"].max(axis=1) - e["E"][np.arange(len(w)), -w]
    return float((err / e["tol_c"]).max()), float((gap / e["tol_E"]).max()), (c, w, h, eq)


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_estimator_within_its_bounds(sps):
    """|c - c64| <= 1.001 * 42 u S1[d] Ymax per component against the float64 least-squares solve (no table in it), and the window the
    model takes has E64[w] >= max E64 - tolE; the taps it hands on are c[w..w+4]."""
    f = batch(sps)
    rc, rE, (c, w, h, eq) = estimator_ratios(f)
    assert np.array_equal(w, f["want"]["win"][eq]) and f["want"]["chan"][eq].tobytes() == h.tobytes()
    rows = np.arange(len(w))[:, None]
    assert np.array_equal(h, c[rows, (w + 4)[:, None] + np.arange(5)[None, :]])
    print("estimator (CPU), sps %d: worst |c - c64| / tol_c = %.3f, worst window gap / tolE = %.3g" % (sps, rc, rE))
    assert rc <= 1.0 and rE <= 1.0


# ---- mutants: the comparison can fail ----
def soft_ratio(f, **mutant):
    """The worst |soft - clamp(soft64)| / bound of the model with one change, graded as the model itself is: its soft bits against
    the reference on its own window and taps."""
    y = f["want"]["y"][f["want"]["win"] <= 0]
    soft, win, h = model.equalise(y, **mutant)
    assert np.all(win <= 0)
    g = ref.grade(soft, soft > 0.5, y, win, h)
    return float(g["ratio"].max())


TRELLIS_MUTANTS = {
    "start state bit-reversed": dict(start=1),                 # a[45], a[46], a[47], a[48] bit 0 first
    "tail not forced": dict(force_tail=False),
    "sign of w": dict(sign_w=-1),                              # y[m - w]
}


@pytest.mark.parametrize("name", sorted(TRELLIS_MUTANTS))
def test_trellis_mutant_is_caught(name):
    """Each changed trellis is at least 100 bounds away from the reference on the mixed batch at sps 4 (the unchanged one is inside)."""
    f = batch(4)
    assert soft_ratio(f) <= 1.0
    worst = soft_ratio(f, **TRELLIS_MUTANTS[name])
    print("mutant %-26s worst |soft - clamp(soft64)| / bound = %.3g" % (name, worst))
    assert worst > 100.0


def test_shifted_table_row_is_caught():
    """One row of P32 moved by one position (the tap's column of A against the wrong symbols): that tap is at least 100 bounds from the
    float64 least-squares solution."""
    P = np.array(model.pinv_table())
    P[6] = np.roll(P[6], 1)
    f = batch(4)
    assert estimator_ratios(f)[0] <= 1.0
    worst = estimator_ratios(f, P)[0]
    print("mutant P32 row shifted       worst |c - c64| / tol_c = %.3g" % worst)
    assert worst > 100.0


# ---- what it buys ----
@pytest.fixture(scope="module")
def fo():
    return fecbind.FecOracle()


def chains(sps, profile, snr, seed, fo):
    """60 seeded bursts with a delay of 0..29 symbols, detectRACHBurst at its default threshold, then demodulateBurst and the model on
    the detected ones: (detected, payload errors demod, model, bursts decoded demod, model) -- decoded = the RACH decoder's tail
    check passes and RA and BSIC are the ones sent."""
    o, bits, ra, bsic, xs, amp, toa, ok = family.static_family(sps, profile, snr, 60, seed)
    x, off, length = mlse_family.pack(xs)
    r = model.access_batch(sps, x, off, length, amp, toa, enable=ok.astype(np.uint8), oracle=o)
    dem = np.stack([o.demodulate(xs[b], amp[b], toa[b])[:148] if ok[b] else np.zeros(148, np.float32) for b in range(60)])
    P = family.PAYLOAD
    errs = [int(((s[ok][:, P] > 0.5) != (bits[ok][:, P] != 0)).sum()) for s in (dem, r["soft"])]
    good = [int(((d[:, 0] != 0) & (d[:, 1] == bsic[ok]) & (d[:, 2] == ra[ok])).sum())
            for d in (fo.rach_decode_batch(dem[ok]), fo.rach_decode_batch(r["soft"][ok]))]
    return int(ok.sum()), errs[0], errs[1], good[0], good[1]


@pytest.mark.parametrize("sps", [1, 4])
@pytest.mark.parametrize("profile", ["five", "precursor", "flat"])
def test_what_it_buys(fo, sps, profile):
    """At 15 dB, on the detected bursts of 60: with `five` and `precursor` the model's payload bit errors are strictly fewer than the
    demodulator's, with `flat` no more; the RACH decoder recovers RA and BSIC from at least as many bursts as from the demodulator's
    soft bits, from strictly more on `five`.  Counts on this seed (detected; errors demodulator -> model of 36 per burst; bursts
    decoded demodulator -> model):
        sps 1  five 37: 129 -> 0, 27 -> 37   precursor 47: 75 -> 0, 43 -> 47   flat 60: 0 -> 0, 60 -> 60
        sps 4  five 31:  76 -> 0, 28 -> 31   precursor 45: 16 -> 0, 45 -> 45   flat 60: 0 -> 0, 60 -> 60"""
    det, e_dem, e_eq, ok_dem, ok_eq = chains(sps, profile, 15.0, 7000 + sps, fo)
    print("sps %d %-9s 15 dB: %d detected; payload errors demodulator %d, equaliser %d of %d; decoded demodulator %d, equaliser %d"
          % (sps, profile, det, e_dem, e_eq, det * 36, ok_dem, ok_eq))
    assert det >= 25
    if profile == "flat":
        assert e_eq <= e_dem
    else:
        assert e_eq < e_dem
    assert ok_eq >= ok_dem
    if profile == "five":
        assert ok_eq > ok_dem
