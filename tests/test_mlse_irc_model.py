"""The interference-rejection equaliser's float32 model (tests/mlse_irc_model.py) on the CPU: the identities against the diversity
model (tests/mlse_div_model.py) and the one-antenna model (tests/mlse_model.py), the antenna swap within the graded bound, the
fallbacks and the given sets that must be refused, the model graded by the float64 reference (tests/mlse_irc_ref.py: the soft
bits and the residual sums, each within its a-priori bound) with three mutants the grading must catch, and what it is for: fewer
payload bit errors than maximal-ratio combining under a co-channel interferer, no more without one.  No GPU: the kernel is held to
this model word for word in tests/test_gpu_mlse_irc.py."""
import numpy as np
import pytest

import mlse_div_family as dfam
import mlse_div_model as dm
import mlse_family
import mlse_irc_family as ifam
import mlse_irc_model as im
import mlse_irc_ref as iref
import mlse_ref
from mlse_variant import variant

F = np.float32


def identity_sets(B):
    return np.tile(im.IDENTITY, (B, 1))


# ---- the identities ----
@pytest.mark.parametrize("sps", [1, 4])
def test_identity_set_is_the_diversity_equaliser(sps):
    """d_cov_in = (1, 1, 0, 0) on every burst: soft bits, hard bits, the window and the taps are mlse_div_model's bit for bit, on
    bursts with and without an interferer; the set that comes back is the identity set.  With the estimated set the soft bits
    are others."""
    f = ifam.mixed_batch(sps, 2, 11, 6300 + 10 * sps + 2)
    div = f["want_div"]
    got = im.mlse_irc_batch(sps, f["x0"], f["off0"], f["x1"], f["off1"], f["length"], f["tsc"], f["amp"], f["toa"], primary=f["primary"],
                            cov_in=identity_sets(11), y=div["y"])
    assert (div["win"] <= 0).sum() >= 9
    for k in ("soft", "hard", "win", "chan"):
        assert got[k].tobytes() == div[k].tobytes(), k
    assert np.array_equal(got["cov"][div["win"] <= 0], identity_sets(int((div["win"] <= 0).sum())))
    assert (f["want"]["soft"] != div["soft"]).any(axis=1).sum() >= 9 and np.array_equal(f["want"]["win"], div["win"])
    assert f["want"]["chan"].tobytes() == div["chan"].tobytes()           # d_chan reports the unwhitened taps


@pytest.mark.parametrize("sps", [1, 4])
def test_second_antenna_all_zeros(sps):
    """Antenna 1 all zeros.  loading == 0: det is 0, the identity set is taken, and everything equals the one-antenna model on
    antenna 0 bit for bit.  loading > 0: the set (1 + loading, loading, 0, 0) is used, and the soft bits agree with the one-antenna
    model's only up to det's roundings -- the float64 reference grades them."""
    f = mlse_family.mixed_batch(sps, 2, 67, 4100 + sps)
    one = f["want"]
    B = len(f["off"])
    y = np.stack([one["y"], np.zeros_like(one["y"])], axis=1)
    zeros = np.zeros_like(f["x"])
    got = im.mlse_irc_batch(sps, f["x"], f["off"], zeros, f["off"], f["length"], f["tsc"], f["amp"], f["toa"], loading=0.0, y=y)
    eq = one["win"] <= 0
    assert eq.sum() >= 60
    assert got["soft"].tobytes() == one["soft"].tobytes() and got["hard"].tobytes() == one["hard"].tobytes()
    assert np.array_equal(got["win"], one["win"])
    assert got["chan"][:, 0].tobytes() == one["chan"].tobytes() and not got["chan"][:, 1].any()
    assert np.array_equal(got["cov"][eq], identity_sets(int(eq.sum()))) and not got["cov"][~eq].any()
    lo = im.mlse_irc_batch(sps, f["x"], f["off"], zeros, f["off"], f["length"], f["tsc"], f["amp"], f["toa"], loading=0.25, y=y)
    noisy = eq & (got["sums"][:, 0] > 0)                       # (a burst that fits its taps exactly has tt = 0: the identity set)
    assert noisy.sum() >= 40
    assert np.array_equal(lo["cov"][noisy], np.tile(np.array([1.25, 0.25, 0.0, 0.0], F), (int(noisy.sum()), 1)))
    assert np.array_equal(lo["win"], one["win"])
    iref.check(lo["soft"][noisy], lo["hard"][noisy], y[noisy], lo["win"][noisy], lo["chan"][noisy], lo["cov"][noisy], f["tsc"], "zeros, loading 0.25")
    assert np.abs(lo["soft"][eq].astype(np.float64) - one["soft"][eq]).max() < 1e-3


@pytest.mark.parametrize("sps", [1, 4])
def test_antennas_swapped_within_the_bound(sps):
    """The LDL form is not symmetric in the antennas: with the antennas exchanged (d_primary too) the soft bits are not the same
    words, but both runs lie within the reference's bound of ITS soft bits for that run, and the two references agree to float64
    accuracy -- the statement is symmetric, the arithmetic is not.  The window is the same; the tap sets are exchanged."""
    f = ifam.mixed_batch(sps, 2, 11, 6300 + 10 * sps + 2)
    a = f["want"]
    b = im.mlse_irc_batch(sps, f["x1"], f["off1"], f["x0"], f["off0"], f["length"], f["tsc"], f["amp"], f["toa"], primary=1 - f["primary"],
                          y=a["y"][:, ::-1])
    assert np.array_equal(a["win"], b["win"])
    assert b["chan"][:, 0].tobytes() == a["chan"][:, 1].tobytes() and b["chan"][:, 1].tobytes() == a["chan"][:, 0].tobytes()
    eq = a["win"] <= 0
    ga = iref.check(a["soft"][eq], a["hard"][eq], a["y"][eq], a["win"][eq], a["chan"][eq], a["cov"][eq], f["tsc"], "antennas as given")
    gb = iref.check(b["soft"][eq], b["hard"][eq], b["y"][eq], b["win"][eq], b["chan"][eq], b["cov"][eq], f["tsc"], "antennas swapped")
    # the two statements are one: e^H R^-1 e, scaled by A det in one run and by Bv det in the other -- and soft64 is a ratio
    sa, sb = ga["ref"]["soft"][:, mlse_family.PAYLOAD], gb["ref"]["soft"][:, mlse_family.PAYLOAD]      # (a known tail symbol is -inf)
    assert np.isfinite(sa).all() and np.abs(sa - sb).max() <= 1e-9 * max(1.0, np.abs(sa).max())
    both = np.abs(a["soft"][eq].astype(np.float64) - b["soft"][eq])[:, mlse_ref.TRELLIS]
    assert np.all(both <= (ga["ref"]["bound"] + gb["ref"]["bound"])[:, mlse_ref.TRELLIS])
    assert a["soft"][eq].tobytes() != b["soft"][eq].tobytes()
    assert a["soft"][:, 61:87].tobytes() == b["soft"][:, 61:87].tobytes()      # the midamble: the same (unwhitened) primary antenna


# ---- the fallbacks, the sets that are refused ----
@pytest.mark.parametrize("sps", [1, 4])
def test_fallbacks_are_the_diversity_equalisers(sps):
    """mlse_div_model's fallback cases (a NaN on the non-primary antenna, an infinity, a 147-symbol burst, zero energy on both
    antennas, d_enable == 0, a refused offset): window words, soft bits and taps are that model's, and the set that comes back is
    zeros; the bursts between them are equalised with a set of their own."""
    f = dfam.mixed_batch(sps, 2, 9, 6200 + sps)
    B = 9
    x0, x1 = f["x0"].copy(), f["x1"].copy()
    length = f["length"].copy(); off0 = f["off0"].copy(); off1 = f["off1"].copy()
    primary = np.array([0, 0, 1, 1, 0, 1, 0, 0, 1], np.uint8)
    enable = np.ones(B, np.uint8)
    x1[off1[1] + 70 * sps + 1:off1[1] + 71 * sps + 1] = np.complex64(complex(np.nan, 1.0))
    x0[off0[2] + 30 * sps:off0[2] + 31 * sps] = np.complex64(complex(0.0, np.inf))
    length[3] = 147 * sps
    x0[off0[4]:off0[4] + length[4]] = 0; x1[off1[4]:off1[4] + length[4]] = 0
    enable[6] = 0
    off1[7] = -1
    div = dm.mlse_div_batch(sps, x0, off0, x1, off1, length, f["tsc"], f["amp"], f["toa"], primary=primary, enable=enable)
    got = im.mlse_irc_batch(sps, x0, off0, x1, off1, length, f["tsc"], f["amp"], f["toa"], primary=primary, enable=enable, y=div["y"])
    assert np.array_equal(got["win"], div["win"]) and got["win"][[1, 2, 3, 4]].tolist() == [1] * 4 and got["win"][[6, 7]].tolist() == [2, 2]
    assert got["chan"].tobytes() == div["chan"].tobytes()
    for b in (1, 2, 3, 4, 6, 7):
        same = (got["soft"][b] == div["soft"][b]) | (np.isnan(got["soft"][b]) & np.isnan(div["soft"][b]))
        assert same.all() and not got["cov"][b].any(), b
    for b in (0, 5, 8):
        assert got["cov"][b, 0] > 0 and got["cov"][b, 1] > 0 and (got["soft"][b] != div["soft"][b]).any()
        assert got["soft"][b, 61:87].tobytes() == div["soft"][b, 61:87].tobytes()


INVALID_SETS = [(np.nan, 1.0, 0.0, 0.0), (1.0, np.nan, 0.0, 0.0), (1.0, 1.0, np.nan, 0.0), (1.0, 1.0, 0.0, np.nan), (1024.0, 1.0, 0.0, 0.0),
                (1.0, 1024.0, 0.0, 0.0), (1.0, 1.0, -1024.0, 0.0), (1.0, 1.0, 0.0, 1024.0), (-1.0, -1.0, 0.0, 0.0), (-1.0, 1.0, 0.0, 0.0),
                (1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 0.8, 0.7), (0.0, 0.0, 0.0, 0.0), (np.inf, 1.0, 0.0, 0.0)]
VALID_SETS = [(1.0, 1.0, 0.0, 0.0), (1023.0, 1023.0, 1000.0, -200.0), (0.5, 2.0, 0.3, -0.4), (2.0 ** -20, 2.0 ** -18, 0.0, 0.0)]
# (not (2^-20, 2^-20, 0, 0): a power of two on both diagonals scales every metric and E_w exactly, and the soft bits are the identity set's)


def test_invalid_given_sets_take_the_identity_set():
    """A NaN, 2^10, a negative diagonal, det <= 0: the identity set is taken (and reported), and the outputs are the diversity
    model's.  The valid sets beside them are used as given."""
    sps = 4
    f = ifam.mixed_batch(sps, 2, 11, 6300 + 10 * sps + 2)
    div = f["want_div"]
    b = int(np.argmax(div["win"] <= 0))
    sets = np.array(INVALID_SETS + VALID_SETS, F)
    n = len(sets)
    rep = lambda a: np.repeat(a[b:b + 1], n, axis=0)
    y = rep(div["y"])
    r = im.equalise(y, f["tsc"], rep(f["primary"]), cov_in=sets)
    k = len(INVALID_SETS)
    assert np.array_equal(r["cov"][:k], identity_sets(k))
    assert np.array_equal(r["cov"][k:], sets[k:])
    for i in range(k + 1):                                     # (the first valid set is the identity set itself)
        assert r["soft"][i].tobytes() == div["soft"][b].tobytes(), INVALID_SETS[i] if i < k else "identity"
    for i in range(k + 1, n):
        assert r["soft"][i].tobytes() != div["soft"][b].tobytes() and np.isfinite(r["soft"][i]).all()


def test_zero_whitened_energy_takes_the_identity_set():
    """A valid set under which E_w underflows to 0 (taps of 2^-60, a set of 2^-20: pw = 2^-40 * 2^-120 + ...): the burst takes the
    identity set after all and E_w is E -- the outputs are the diversity model's."""
    y = np.zeros((1, 2, 148), np.complex64)
    t = im.tsc_symbols(3)
    base = np.zeros(148); base[61:87] = t
    rng = np.random.default_rng(5)
    base[:61] = rng.choice([-1.0, 1.0], 61); base[87:] = rng.choice([-1.0, 1.0], 61)
    y[0, 0] = (base * 2.0 ** -60).astype(np.complex64); y[0, 1] = (1j * base * 2.0 ** -60).astype(np.complex64)
    soft, win, h = dm.equalise(y, 3)
    assert win[0] <= 0
    r = im.equalise(y, 3, cov_in=np.array([[2.0 ** -20, 2.0 ** -20, 0.0, 0.0]], F))
    assert np.array_equal(r["cov"], identity_sets(1)) and r["soft"].tobytes() == soft.tobytes() and r["Ew"][0] > 0


# ---- graded by the float64 reference ----
def graded(sps):
    return ifam.graded_batch(sps, per=24 if sps == 1 else 8)


@pytest.mark.parametrize("sps", [1, 4])
def test_model_within_the_bounds(sps):
    """72 bursts at sps 1 (24 at sps 4), independent channels per antenna, clean, 15 dB and 8 dB, an interferer on five of six: no
    bad_soft, bad_clamp or bad_hard anywhere, at most 0.5 % of a noise level's payload positions outside the hard-bit comparison;
    S00, S11, Xr and Xi within their bound of the float64 sums.  Measured on the CPU (sps 1 / sps 4): worst |soft - clamp(soft64)| /
    bound 0.0042 / 0.0035; worst |S - S64| / bound 0.096 / 0.071."""
    f = graded(sps)
    wt = f["want"]
    eq = wt["win"] <= 0
    assert eq.sum() >= len(eq) - 2 and (sps != 1 or len(eq) >= 64)
    assert (np.abs(wt["cov"][eq][:, 2:]).max(axis=1) > 0.05).sum() >= eq.sum() // 2          # the sets are not the identity set
    g = iref.check(wt["soft"][eq], wt["hard"][eq], wt["y"][eq], wt["win"][eq], wt["chan"][eq], wt["cov"][eq], f["tsc"], "model, sps %d" % sps)
    tally = mlse_ref.Tally(mlse_family.PAYLOAD)
    tally.add(g, f["snr"][eq], f["group"][eq])
    tally.report("IRC model (CPU), sps %d" % sps)
    tally.assert_cap("IRC model, sps %d" % sps)
    worst = iref.check_sums(wt["sums"][eq], wt["y"][eq], wt["win"][eq], wt["chan"][eq], f["tsc"], "model, sps %d" % sps)
    print("IRC model (CPU), sps %d: worst |soft - clamp(soft64)| / bound = %.4f, worst |S - S64| / bound = %.4f" % (sps, g["ratio"].max(), worst))


MUTANTS = {
    "wrong sign of xi in the whitening": ("wi = A * v1i - (xr * v0i - xi * v0r)", "wi = A * v1i - (xr * v0i + xi * v0r)"),
    "det left off antenna 0's metric": ("g = det[:, None] * (dr0 * dr0 + di0 * di0) + (dr1 * dr1 + di1 * di1)",
                                        "g = (dr0 * dr0 + di0 * di0) + (dr1 * dr1 + di1 * di1)"),
    "E in place of E_w": ("den_E = Ew.astype(F)", "den_E = E.astype(F)"),
    "loading left off Bv": ("Bv = S11 / tt + F(loading)", "Bv = S11 / tt"),
}
WIDE = 20.0                                                    # "a wide factor": what a mutant must exceed the bound by


def worst_ratio(model, f):
    """The variant's soft bits against the reference on the set the TRUE model used (a mutant that changes the set is graded on
    what the set should have been)."""
    r = model.equalise(f["want"]["y"], f["tsc"], f["primary"])
    wt = f["want"]
    eq = wt["win"] <= 0
    g = iref.grade(r["soft"][eq], r["soft"][eq] > 0.5, wt["y"][eq], wt["win"][eq], wt["chan"][eq], wt["cov"][eq], f["tsc"])
    return float(g["ratio"].max())


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_is_caught(name):
    """Each mutant exceeds the bound on the graded family by more than a factor of 20 (the unmutated copy, built the same way, stays
    inside)."""
    f = graded(1)
    if name == sorted(MUTANTS)[0]:
        assert worst_ratio(variant(im), f) <= 1.0
    worst = worst_ratio(variant(im, MUTANTS[name]), f)
    print("mutant %-36s worst |soft - clamp(soft64)| / bound = %.3g" % (name, worst))
    assert worst > WIDE


# ---- what it is for ----
CASES = {   # name: (family, IRC's errors at most this fraction of MRC's)
    "C/I 3 dB, SNR 25 dB, five-tap interferer": (lambda: ifam.interfered_family(4, 3.0, 25.0, 60, 2), 0.75),
    "C/I 0 dB, SNR 25 dB, one-tap interferer": (lambda: ifam.interfered_family(4, 0.0, 25.0, 60, 4, iprofile=(1.0,)), 0.6),
    "no interferer, SNR 9 dB": (lambda: dfam.rayleigh_family(4, 9.0, 60, 31), 1.05),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_rejection_pays(name):
    """sps 4, 60 bursts of the "five" profile with independent Rayleigh taps per antenna and burst, loading 1/64, an undetected burst
    counting as half its payload bits; payload bit errors of 6,960, MRC (mlse_div_model) against IRC.  Counted on this CPU:
        C/I 3 dB, SNR 25 dB, five-tap interferer (seed 2)   MRC 570, IRC 347 (0.61)
        C/I 0 dB, SNR 25 dB, one-tap interferer (seed 4)    MRC 1287, IRC 553 (0.43)
        no interferer, SNR 9 dB (rayleigh_family, seed 31)  MRC 64, IRC 65 (1.02)
    IRC's count is at most 3/4, 0.6 and 1.05 of MRC's; MRC makes at least 50 errors in each, so that the comparison is not empty."""
    family, cap = CASES[name]
    mrc, irc, lost = ifam.payload_errors(family())
    print("%s: MRC %d, IRC %d (%.2f) of 6960 payload bits; neither antenna detected: %d bursts" % (name, mrc, irc, irc / max(mrc, 1), lost))
    assert mrc >= 50
    assert irc <= cap * mrc
