"""The fit detector's float32 model (tests/sch_fit_model.py) on the CPU: graded against the float64 statement (tests/sch_fit_ref.py)
within the a-priori bound, with three one-change mutants outside it; the measurement behind TRXSIG_L1ACQ_SCH_FIT_THRESH; what the
detector buys on the static multipath families; and a whole search with the fit verdict.  No GPU.

Measured (float32 model, this file's seeds; the header and DESIGN.md 5.4.vi carry the same figures):
  worst error / bound on 37 bursts a rate: R 0.037, 0.048, 0.032 and q 0.076, 0.051, 0.044 at sps 1, 2, 4.
  (a) the largest q on candidate windows without an SCH: 0.9227 at sps 1 (2,803 candidates of 28,601 windows: random bits through
      the five-tap channel), 0.8736 at sps 4 (2,720 of 28,601).
  (b) the smallest q on 60 SCH windows a profile at 10 dB: sps 1 flat 2.686, five 2.176, precursor 2.062; sps 4 2.816, 2.093, 2.493.
  (b) / (a) = 2.234 (required: 1.5); sqrt(a b) = 1.379; the constant is 1.4.
  At 6 dB the smallest q: sps 1 1.692, 1.374, 1.443; sps 4 1.735, 1.519, 1.652 (flat, five, precursor): the detector begins to miss.
  At 15 dB: sps 1 5.036, 2.883, 2.951; sps 4 4.777, 3.581, 4.445."""
import functools

import numpy as np
import pytest

import l1_acq_model as am
import mlse_sch_family as fam
import sch_fit_family as ff
import sch_fit_model as model
import sch_fit_ref as ref

THRESH = 1.4                                                  # TRXSIG_L1ACQ_SCH_FIT_THRESH
ROUNDS = 2200                                                 # windows per class of set (a): 28,601 windows a rate
PROFILES = ("flat", "five", "precursor")
F = np.float32


@functools.lru_cache(maxsize=None)
def graded(sps):
    f = fam.mixed_batch(sps, 37, 6100 + sps)
    r = model.fit_batch(sps, f["x"], f["off"], f["length"], f["amp"], f["toa"])
    on = r["win"] <= 0
    assert on.sum() >= 33
    return f, r, on


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_model_within_the_float64_bound(sps):
    f, r, on = graded(sps)
    assert np.array_equal(r["win"], f["want"]["win"]) and np.array_equal(r["chan9"][np.arange(37)[:, None], (r["w"] + 4)[:, None] + np.arange(5)][on],
                                                                         f["want"]["chan"][on])      # the equaliser's window and taps
    g = ref.grade(r["R"][on], r["q"][on], r["y"][on], r["w"][on], r["h"][on])
    print("sps %d: worst error / bound on %d bursts: R %.3f, q %.3f; q from %.3g to %.3g" % (sps, on.sum(), g["ratio_R"].max(), g["ratio_q"].max(),
                                                                                           r["q"][on].min(), r["q"][on].max()))
    assert np.isfinite(g["ref"]["bound_q"]).all()
    assert g["ok_R"].all() and g["ok_q"].all(), (g["ratio_R"].max(), g["ratio_q"].max())
    assert np.allclose(r["E"][on], g["ref"]["E"], rtol=6 * ref.U * ref.SLACK, atol=0)


@pytest.mark.parametrize("sps", [1, 4])
def test_mutants_land_outside_the_bound(sps):
    """A window off by one (the signs taken for w - 1, or w + 1 where w = -4), a sign of a taken from n - w - k + 1, and the
    reduction dropping row 101: the first two move R and q of EVERY graded burst outside the bound; the dropped row does so on
    every burst whose bound resolves one row of 56 (bR < 1e-4 R: the noisy and the multipath bursts -- on a noise-free burst the
    residual is itself rounding error, q is some 10^5, and the bound is as large as R; that is the bound's honest answer there)."""
    f, r, on = graded(sps)
    base = ref.fit64(r["y"][on], r["w"][on], r["h"][on])
    sharp = base["bound_R"] < 1e-4 * base["R"]
    assert sharp.sum() >= 20, sharp.sum()
    shift = np.where(r["w"] > -4, -1, 1)
    y = r["y"]
    muts = {"window": lambda: model.tree(model.row_energies(y, r["w"] + shift, r["h"])),
            "sign": lambda: model.tree(model.row_energies(y, r["w"], r["h"], sign_shift=1)),
            "row101": lambda: model.tree(model.row_energies(y, r["w"], r["h"]), drop_last=True)}
    for name, fn in muts.items():
        R = fn()
        q = model.quality(r["E"], R)
        g = ref.grade(R[on], q[on], y[on], r["w"][on], r["h"][on])
        print("sps %d mutant %s: smallest error / bound: R %.3g, q %.3g" % (sps, name, g["ratio_R"].min(), g["ratio_q"].min()))
        which = sharp if name == "row101" else np.ones_like(sharp)
        assert not g["ok_R"][which].any() and not g["ok_q"][which].any(), name
    assert np.array_equal(model.tree(model.row_energies(y, r["w"], r["h"]))[on], r["R"][on])


def test_edges_of_the_statement():
    """R == 0 with E > 0 gives +inf and keeps it; 0 / 0 and NaN give 0; an all-zero burst, a component of 2^30 and a NaN fall back."""
    E = np.array([1.0, 0.0, np.nan, 4.0], F); R = np.array([0.0, 0.0, 1.0, 51.0], F)
    q = model.quality(E, R)
    assert q[0] == np.inf and q[1] == 0 and q[2] == 0 and q[3] == 2.0
    # a burst the five taps fit exactly: y = sum h a with h on a power-of-two grid (every sum exact)
    h = np.array([[0.5, -0.25j, 0.125, 0, 0]], np.complex64)
    a = model.A_SIGN.astype(np.float64)
    y = np.zeros((1, 148), np.complex64)
    for n in range(46, 102):
        y[0, n] = sum(h[0, k] * a[n - k] for k in range(5))
    e = model.row_energies(y, np.array([0]), h)
    assert not e.any() and model.quality(np.array([1.0], F), model.tree(e))[0] == np.inf
    z = np.zeros((3, 148), np.complex64)
    z[1, 50] = 2.0 ** 30; z[2, 60] = np.nan
    r = model.fit(z)
    assert (r["win"] == 1).all() and not r["q"].any() and not r["R"].any() and not r["E"].any() and not r["chan9"].any()


@functools.lru_cache(maxsize=None)
def measured():
    a = {sps: ff.negative_set(sps, ROUNDS) for sps in (1, 4)}
    b = {(sps, p, snr): ff.positive_q(sps, p, snr) for sps in (1, 4) for p in PROFILES for snr in (15.0, 10.0, 6.0)}
    return a, b


def test_threshold_measurement():
    """Section (a), (b) of the header's measurement, asserted with the committed constant (the figures: this file's docstring)."""
    a, b = measured()
    for sps in (1, 4):
        kinds = set(a[sps]["kind"])
        print("sps %d (a): %d windows, %d candidates, largest q %.4f; classes seen: %s" % (sps, a[sps]["n_windows"], a[sps]["n_candidates"],
                                                                                          a[sps]["q"].max(), sorted(kinds)))
        assert a[sps]["n_candidates"] >= 2000 and "noise" in kinds and any(k.startswith("random/") for k in kinds) and any(k.startswith("dummy/") for k in kinds)
    amax = max(float(a[sps]["q"].max()) for sps in (1, 4))
    for snr in (15.0, 10.0, 6.0):
        for sps in (1, 4):
            print("sps %d %4.1f dB smallest / median q: " % (sps, snr) + ", ".join("%s %.3f / %.3f" % (p, b[sps, p, snr]["q"].min(), np.median(b[sps, p, snr]["q"]))
                                                                                  for p in PROFILES))
    bmin = min(float(b[sps, p, 10.0]["q"].min()) for sps in (1, 4) for p in PROFILES)
    assert all(b[sps, p, 10.0]["candidate"].all() for sps in (1, 4) for p in PROFILES)
    gm = float(np.sqrt(amax * bmin))
    print("(a) %.4f (b) %.4f ratio %.3f geometric mean %.4f" % (amax, bmin, bmin / amax, gm))
    assert bmin / amax >= 1.5
    assert float("%.2g" % gm) == THRESH
    assert amax < THRESH < bmin


@pytest.mark.parametrize("sps", [1, 4])
def test_what_it_buys(sps):
    """static_family at 15 and 10 dB: FIT at its constant detects at least as many windows as VALLEY at 8.0 on every profile and
    all 60 on flat, and none of set (a); with the equaliser behind it, it decodes (right FN and BSIC) no fewer bursts than VALLEY
    with the demodulator."""
    a, b = measured()
    assert not (a[sps]["q"] > F(THRESH)).any()
    det_v, det_fm = fam.detector(sps), ff.fit_detector(sps, True)
    for snr in (15.0, 10.0):
        for p in PROFILES:
            m = b[sps, p, snr]
            fit = m["q"] > F(THRESH)
            assert fit.sum() >= m["valley"].sum() and (p != "flat" or fit.all()), (snr, p)
            o, bits, fn, bsic, xs = m["family"][:5]
            good = {"VALLEY+DEMOD": 0, "FIT+MLSE": 0}
            for i, x in enumerate(xs):
                for name, det, th in (("VALLEY+DEMOD", det_v, 8.0), ("FIT+MLSE", det_fm, THRESH)):
                    r = det.detect(x, None, th)
                    good[name] += int(bool(r["flags"] & 2) and fam.decode(r["soft"]) == (True, int(bsic[i]), int(fn[i])))
            print("sps %d %s %4.1f dB: detected VALLEY %2d FIT %2d of 60; decoded with the right FN and BSIC: VALLEY+DEMOD %2d, FIT+MLSE %2d"
                  % (sps, p, snr, m["valley"].sum(), fit.sum(), good["VALLEY+DEMOD"], good["FIT+MLSE"]))
            assert good["FIT+MLSE"] >= good["VALLEY+DEMOD"], (snr, p, good)


@pytest.mark.parametrize("sps", [1, 4])
def test_search_with_the_fit_verdict(sps):
    """l1_acq_model.search_model with the fit detector on tests/mlse_sch_family.search_streams (three symbols of spread, 12 dB) at
    the DEFAULT thresholds: state 15 with the right FN and BSIC on every stream for FIT + MLSE, on none for VALLEY + MLSE (which
    stops at state 3); the negative streams reach no state bit 4."""
    tx = fam._tx()
    n15 = {}
    for name, det, th in (("VALLEY", fam.MlseSchDetector(fam.detector(sps).o), 8.0), ("FIT", ff.fit_detector(sps, True), THRESH)):
        n15[name] = 0
        for x, case in fam.search_streams(sps):
            r = am.search_model(det, tx, x, 0.5, th)
            if r["state"] == 15:
                at = r["w0"] + float(r["sch"]["toa"])
                fn = min(case["sch"], key=lambda p: abs(p[1] - at))[0]
                n15[name] += int((r["bsic"], r["rfn"]) == (case["bsic"], fn))
    print("sps %d: streams at state 15 with the right FN and BSIC: VALLEY + MLSE %d, FIT + MLSE %d of 4" % (sps, n15["VALLEY"], n15["FIT"]))
    assert n15["FIT"] == 4 and n15["VALLEY"] < n15["FIT"]
    for name, x in am.negative_streams(fam.detector(sps).o, tx, sps):
        assert not am.search_model(ff.fit_detector(sps, True), tx, x, 0.5, THRESH)["state"] & 4, name
