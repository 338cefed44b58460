"""The synchronisation-burst sequence equaliser's float32 model (tests/mlse_sch_model.py): its least-squares table from Python
integers (its trellis is every model's: tests/test_mlse_core.py), the model graded against the float64 reference
(tests/mlse_sch_ref.py) within the bounds derived there, the one-tap channel against the demodulator's formula, five one-change
mutants that the grading must catch, and what the equaliser buys over demodulateBurst behind acquisition's SCH detector on seeded
multipath families.  No GPU: tests/test_gpu_mlse_sch.py holds the kernel to the model word for word,
tests/test_gpu_mlse_sch_ref.py to the reference."""
import numpy as np
import pytest

import mlse_family
import mlse_model
import mlse_sch_family as family
import mlse_sch_model as model
import mlse_sch_ref as ref

B_ALL = 37
F = np.float32


def batch(sps):
    return family.mixed_batch(sps, B_ALL, 6100 + sps)          # (shared with the GPU tests: computed once per process)


# ---- the table ----
def test_table_from_integers():
    """G = A^T A is 56 on the diagonal and at most 6 off it; det(G) and max |adj(G) A^T| are the two integers the design was checked
    with, both below 2^53, so the double division and the float32 rounding are each ONE correct rounding; |P32| < 0.0253; the rows
    of P32 sum to at most 1.0001 in magnitude (the header's finiteness argument); P32 A is the identity to within the roundings of
    P32's entries: entry (d, e) of P32 A - I is sum_j (P32 - P)[d][j] A[j][e] with |A| = 1 and |P32 - P| <= 2^-25 |P|, so it is at
    most 1.001 * 2^-25 * sum_j |P[d][j]| over the 56 terms -- evaluated here in exact rational arithmetic."""
    from fractions import Fraction
    A = model.design_matrix()
    assert len(A) == 56 and all(len(r) == 9 and set(r) <= {-1, 1} for r in A)
    G = [[sum(A[n][i] * A[n][j] for n in range(56)) for j in range(9)] for i in range(9)]
    assert all(G[i][i] == 56 for i in range(9)) and max(abs(G[i][j]) for i in range(9) for j in range(9) if i != j) <= 6
    N, det = model.pinv_integers()
    assert det == 4848207871868928 and max(abs(v) for row in N for v in row) == 122392273747968
    assert 0 < det < 2 ** 53 and all(abs(v) < 2 ** 53 for row in N for v in row)
    for i in range(9):                                        # N / det IS the pseudo-inverse: (N A) = det * I, exactly
        for e in range(9):
            assert sum(N[i][n] * A[n][e] for n in range(56)) == (det if i == e else 0)
    P32 = model.pinv_table()
    assert P32.shape == (9, 56) and P32.dtype == np.float32 and 0.0252 < np.abs(P32).max() < 0.0253
    for i in range(9):
        for n in range(56):
            assert P32[i, n] == np.float32(np.float64(N[i][n]) / np.float64(det))
    worst = 0.0
    for d in range(9):
        bound = Fraction(1001, 1000) * Fraction(1, 2 ** 25) * sum(abs(Fraction(N[d][j], det)) for j in range(56))
        for e in range(9):
            dev = abs(sum(Fraction(float(P32[d, j])) * A[j][e] for j in range(56)) - int(d == e))
            assert dev <= bound, (d, e, float(dev), float(bound))
            worst = max(worst, float(dev / bound))
    gain = (P32.astype(np.float64) ** 2).sum(axis=1)          # the estimator's noise gain per tap
    S1 = np.abs(P32.astype(np.float64)).sum(axis=1)
    assert 0.01824 <= gain.min() and gain.max() <= 0.01851, gain
    assert 0.9999 <= S1.min() and S1.max() <= 1.0001, S1
    cond = np.linalg.cond(np.array(G, np.float64))
    assert 1.63 < cond < 1.65, cond
    print("P32 A - I: worst entry at %.3f of its bound; noise gain %.5f to %.5f per tap; S1 %.6f to %.6f; cond(G) %.3f"
          % (worst, gain.min(), gain.max(), S1.min(), S1.max(), cond))


def test_start_states():
    """a[105], a[104], a[103], a[102] and a[42], a[43], a[44], a[45], bit 0 first, from the extended training sequence (the kernel's
    two constants are held to these in tests/test_mlse_sch_abi.py)."""
    x = model.XTS
    assert len(x) == 64
    assert model.START_RIGHT == x[63] | x[62] << 1 | x[61] << 2 | x[60] << 3 == 11
    assert model.START_LEFT == x[0] | x[1] << 1 | x[2] << 2 | x[3] << 3 == 13


# ---- the model against the float64 statement ----
@pytest.mark.parametrize("sps", [1, 2, 4])
def test_model_within_the_bound(sps):
    """On positions 0..41 and 106..147 of every burst of the mixed batch: |model soft - clamp(soft64)| <= bound; exactly 0 or 1 where
    soft64 is outside [0, 1] by more than the bound (the six tail bits among them: soft64 = -inf, the model exactly 0); hard bits
    equal wherever |soft64 - 0.5| > bound, and the positions inside that margin are at most 0.5 % of the coded bits.
    Worst |soft - clamp(soft64)| / bound measured: 0.0015 (sps 1), 0.0017 (sps 2), 0.0013 (sps 4)."""
    f = batch(sps)
    wt = f["want"]
    eq = wt["win"] <= 0
    assert eq.sum() >= B_ALL - 2
    g = ref.check(wt["soft"][eq], wt["hard"][eq], wt["y"][eq], wt["win"][eq], wt["chan"][eq], "model, sps %d" % sps)
    tails = [0, 1, 2, 145, 146, 147]
    assert np.all(wt["soft"][eq][:, tails] == 0.0) and np.all(np.isneginf(g["ref"]["soft"][:, tails]))
    ex = int(g["excluded"][:, family.CODED].sum())
    print("model (CPU), sps %d: worst |soft - clamp(soft64)| / bound = %.4f (bound %.2e to %.2e); %d of %d coded positions inside the margin"
          % (sps, g["ratio"].max(), np.nanmin(g["ref"]["bound"]), np.nanmax(g["ref"]["bound"]), ex, eq.sum() * 78))
    assert ex <= 0.005 * eq.sum() * 78


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
    """|c - c64| <= 1.001 * 57 u S1[d] Ymax per component against the float64 least-squares solve (no table in it), and the window the
    model takes has E64[w] >= max E64 - tolE; the taps it hands on are c[w..w+4]."""
    f = batch(sps)
    rc, rE, (c, w, h, eq) = estimator_ratios(f)
    assert np.array_equal(w, f["want"]["win"][eq]) and f["want"]["chan"][eq].tobytes() == h.tobytes()
    rows = np.arange(len(w))[:, None]
    assert np.array_equal(h, c[rows, (w + 4)[:, None] + np.arange(5)[None, :]])
    print("estimator (CPU), sps %d: worst |c - c64| / tol_c = %.3f, worst window gap / tolE = %.3g" % (sps, rc, rE))
    assert rc <= 1.0 and rE <= 1.0


def test_one_tap_channel_is_the_demodulator():
    """With h = (1, 0, 0, 0, 0), w = 0 and E = 1, (M_0 - M_1) / (8 E) is Re(y) / 2: the reference says so to float64's rounding, and
    the model's soft bits lie within the derived bound of the demodulator's formula clamp((y.re + 1) * 0.5) on the coded positions
    4..41 and 106..144 (the six tail bits are forced to 0, where the demodulator only comes near it), with equal hard bits outside
    the margin.  Position 3 is the exception the burst model makes, as in trxsig_mlse_batch: the left half reads y[4 + w ..], so with
    one tap at h[0] and w = 0 nothing it reads holds a[3], and the soft bit is exactly 0.5 in the model and in the reference.  (The
    estimator never leaves it so on a received burst: the modulator's pulse alone puts energy into c[-1], and the window with it wins.)"""
    rng = np.random.default_rng(17)
    B = 12
    bits, _, _ = family.sch_bits(rng, B)
    a = 2.0 * bits.astype(np.float64) - 1.0
    y = (a + 0.35 * (rng.standard_normal((B, 148)) + 1j * rng.standard_normal((B, 148)))).astype(np.complex64)
    h = np.zeros((B, 5), np.complex64); h[:, 0] = 1.0
    w = np.zeros(B, np.int32); E = np.ones(B, F)
    soft = model.trellis(y, w, h, E)
    dem = mlse_model.slicer(y.real.astype(F))
    r = ref.equalise64(y, w, h)
    assert np.all(soft[:, 3] == F(0.5)) and np.all(r["soft"][:, 3] == 0.5)
    C = family.CODED[1:]
    assert np.abs(r["soft"][:, C] - (0.5 + y.real.astype(np.float64)[:, C] / 2.0)).max() <= 1e-12
    dev = np.abs(soft[:, C].astype(np.float64) - dem[:, C].astype(np.float64))
    slack = r["bound"][:, C] + 2.0 ** -24                      # (the demodulator's own two roundings)
    print("one tap: worst |model - demodulator| = %.3g, %.4f of the bound" % (dev.max(), (dev / slack).max()))
    assert np.all(dev <= slack)
    far = np.abs(r["soft"][:, C] - 0.5) > slack
    assert np.array_equal((soft[:, C] > 0.5)[far], (dem[:, C] > 0.5)[far]) and far.mean() > 0.95
    assert np.array_equal(soft[:, 42:106], dem[:, 42:106]) and np.all(soft[:, [0, 1, 2, 145, 146, 147]] == 0.0)


# ---- mutants: the comparison can fail ----
def soft_ratio(f, **mutant):
    """The worst |soft - clamp(soft64)| / bound of the model with one change, graded as the model itself is: its soft bits against
    the reference on its own window and taps."""
    y = f["want"]["y"][f["want"]["win"] <= 0]
    soft, win, h = model.equalise(y, **mutant)
    assert np.all(win <= 0)
    g = ref.grade(soft, soft > 0.5, y, win, h)
    return float(g["ratio"].max())


def _reverse4(s):
    return (s & 1) << 3 | (s & 2) << 1 | (s & 4) >> 1 | (s & 8) >> 3


# how far out each mutant lands on the mixed batch at sps 4, in units of its bound (measured on the CPU model)
MEASURED_RS, MEASURED_LS, MEASURED_TAIL, MEASURED_G, MEASURED_ROW = 2.5e3, 3.49e3, 4.17e3, 8.05e3, 1.86e5
# name -> (the change, that ratio)
TRELLIS_MUTANTS = {
    "right start state bit-reversed": (dict(start_right=_reverse4(model.START_RIGHT)), MEASURED_RS),
    "left start state bit-reversed": (dict(start_left=_reverse4(model.START_LEFT)), MEASURED_LS),
    "tail not forced": (dict(force_tail=False), MEASURED_TAIL),
    "left half's g not reversed": (dict(reverse_left=False), MEASURED_G),
}


@pytest.mark.parametrize("name", sorted(TRELLIS_MUTANTS))
def test_trellis_mutant_is_caught(name):
    """Each changed trellis lands far outside the bound on the mixed batch at sps 4 (the unchanged one is inside).  Worst
    |soft - clamp(soft64)| / bound: right start state bit-reversed 2.5e3, left start state bit-reversed 3.49e3, tail not forced
    4.17e3, the left half's g not reversed 8.05e3.  Asserted is a tenth of each."""
    f = batch(4)
    assert soft_ratio(f) <= 1.0
    change, measured = TRELLIS_MUTANTS[name]
    worst = soft_ratio(f, **change)
    print("mutant %-32s worst |soft - clamp(soft64)| / bound = %.3g" % (name, worst))
    assert worst > measured / 10.0 > 1.0


def test_shifted_table_row_is_caught():
    """One row of P32 moved by one position (the tap's column of A against the wrong symbols): that tap is 1.86e5 bounds from the
    float64 least-squares solution; asserted is a tenth of that."""
    P = np.array(model.pinv_table())
    P[6] = np.roll(P[6], 1)
    f = batch(4)
    assert estimator_ratios(f)[0] <= 1.0
    worst = estimator_ratios(f, P)[0]
    print("mutant P32 row shifted            worst |c - c64| / tol_c = %.3g" % worst)
    assert worst > MEASURED_ROW / 10.0 > 1.0


# ---- what it buys ----
def chains(sps, profile, snr, seed, thresh):
    """60 seeded windows of 172 symbols with the burst 8..16 symbols in, acquisition's SCH detector at `thresh`, then demodulateBurst
    and the model on the detected ones, as stage 2 of trxsig_l1acq calls them (the window from floor(TOA) on, the fraction as the
    TOA): (detected, coded-bit errors demod, model, bursts decoded demod, model) -- decoded = the SCH decoder's parity is good and FN
    and BSIC are the ones sent."""
    o, bits, fn, bsic, xs, amp, toa, ok = family.static_family(sps, profile, snr, 60, seed, thresh=thresh)
    det = family.detector(sps)
    mdet = family.MlseSchDetector(o)
    dem = np.zeros((60, 148), F); eq = np.zeros((60, 148), F)
    for b in range(60):
        if ok[b]:
            dem[b] = det.detect(xs[b], None, thresh)["soft"]
            eq[b] = mdet.detect(xs[b], None, thresh)["soft"]
    C = family.CODED
    errs = [int(((s[ok][:, C] > 0.5) != (bits[ok][:, C] != 0)).sum()) for s in (dem, eq)]
    good = [sum(1 for b in np.flatnonzero(ok) if family.decode(s[b]) == (True, int(bsic[b]), int(fn[b]))) for s in (dem, eq)]
    return int(ok.sum()), errs[0], errs[1], good[0], good[1]


@pytest.mark.parametrize("thresh", [8.0, 3.0])
@pytest.mark.parametrize("sps", [1, 4])
@pytest.mark.parametrize("profile", ["five", "precursor", "flat"])
def test_what_it_buys(sps, profile, thresh):
    """At 15 dB, on the detected bursts of 60, at the detector's default threshold (8.0) and at 3.0.  Counts on this seed (detected;
    coded-bit errors demodulator -> model of 78 per burst; bursts decoded demodulator -> model):
        threshold 8.0   sps 1  five  2:   0 -> 0,  2 ->  2   precursor  0: -                 flat 60: 0 -> 0, 60 -> 60
                        sps 4  five  3:   4 -> 0,  2 ->  3   precursor  0: -                 flat 60: 0 -> 0, 60 -> 60
        threshold 3.0   sps 1  five 51: 369 -> 0, 38 -> 51   precursor 60: 129 -> 0, 56 -> 60   flat 60: 0 -> 0, 60 -> 60
                        sps 4  five 50: 363 -> 0, 39 -> 50   precursor 60:  45 -> 0, 60 -> 60   flat 60: 0 -> 0, 60 -> 60
    At the default threshold the DETECTOR is what multipath breaks: its valley rule counts echoes 2 to 5 symbols beside the peak as
    noise, and hardly a burst of `five` or `precursor` reaches either leg.  Asserted at both thresholds: on `five` and `precursor` the
    equaliser is never worse than the demodulator, in bit errors and in decoded bursts; on `flat` the two are equal; at 3.0 at least
    40 of 60 are detected."""
    det, e_dem, e_eq, ok_dem, ok_eq = chains(sps, profile, 15.0, 8000 + sps, thresh)
    print("sps %d %-9s 15 dB, threshold %.0f: %d detected; coded-bit errors demodulator %d, equaliser %d of %d; decoded demodulator %d, equaliser %d"
          % (sps, profile, thresh, det, e_dem, e_eq, det * 78, ok_dem, ok_eq))
    if thresh < 8.0:
        assert det >= 40
    if profile == "flat":
        assert e_eq == e_dem and ok_eq == ok_dem
    else:
        assert e_eq <= e_dem and ok_eq >= ok_dem
