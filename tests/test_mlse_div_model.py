"""The two-antenna sequence equaliser's float32 model (tests/mlse_div_model.py) on the CPU: the three exact identities against the
one-antenna model (tests/mlse_model.py), every fallback, the selection rule, the model graded by the float64 reference
(tests/mlse_div_ref.py) with two mutants the grading must catch, and what it is for: fewer bit errors than one antenna, no more
than the selected antenna alone.  No GPU: the kernel is held to this model word for word in tests/test_gpu_mlse_div.py."""
import numpy as np
import pytest

import mlse_div_family as dfam
import mlse_div_model as dm
import mlse_div_ref as dref
import mlse_family
import mlse_model as mm
import mlse_ref
import oraclebind
from mlse_variant import variant


def same_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ---- the three identities ----
@pytest.mark.parametrize("sps", [1, 4])
def test_second_antenna_all_zeros(sps):
    """Antenna 1 all zeros: soft bits, hard bits and the window are the one-antenna model's on antenna 0, chan[b][0] its taps,
    chan[b][1] zeros."""
    f = mlse_family.mixed_batch(sps, 2, 67, 4100 + sps)
    want = f["want"]
    got = dm.mlse_div_batch(sps, f["x"], f["off"], np.zeros_like(f["x"]), f["off"], f["length"], f["tsc"], f["amp"], f["toa"])
    assert (want["win"] <= 0).sum() >= 60
    assert got["soft"].tobytes() == want["soft"].tobytes() and got["hard"].tobytes() == want["hard"].tobytes()
    assert np.array_equal(got["win"], want["win"])
    assert got["chan"][:, 0].tobytes() == want["chan"].tobytes() and not got["chan"][:, 1].any()


@pytest.mark.parametrize("sps", [1, 4])
def test_same_samples_on_both_antennas(sps):
    """The same samples twice (at another offset): p, gamma, E and M_0 - M_1 all double exactly -- soft bits, hard bits and the
    window are the one-antenna model's, both tap sets its taps."""
    f = mlse_family.mixed_batch(sps, 2, 67, 4100 + sps)
    want = f["want"]
    x1 = np.concatenate([np.zeros(3, np.complex64), f["x"]])
    got = dm.mlse_div_batch(sps, f["x"], f["off"], x1, f["off"] + 3, f["length"], f["tsc"], f["amp"], f["toa"])
    assert got["soft"].tobytes() == want["soft"].tobytes() and got["hard"].tobytes() == want["hard"].tobytes()
    assert np.array_equal(got["win"], want["win"])
    assert got["chan"][:, 0].tobytes() == want["chan"].tobytes() and got["chan"][:, 1].tobytes() == want["chan"].tobytes()


@pytest.mark.parametrize("sps", [1, 4])
def test_antennas_swapped(sps):
    """Antennas exchanged, d_primary with them: soft bits and the window identical, the two tap sets exchanged."""
    f = dfam.mixed_batch(sps, 2, 33, 6100 + sps)
    want = f["want"]
    assert (want["win"] <= 0).sum() >= 28 and 0 < f["primary"].sum() < 33
    got = dm.mlse_div_batch(sps, f["x1"], f["off1"], f["x0"], f["off0"], f["length"], f["tsc"], f["amp"], f["toa"], primary=1 - f["primary"])
    assert got["soft"].tobytes() == want["soft"].tobytes() and np.array_equal(got["win"], want["win"])
    assert got["chan"][:, 0].tobytes() == want["chan"][:, 1].tobytes() and got["chan"][:, 1].tobytes() == want["chan"][:, 0].tobytes()
    # and the second antenna matters: without it the soft bits are others
    alone = mm.mlse_batch(sps, f["x0"], f["off0"], f["length"], f["tsc"], f["amp"], f["toa"])
    assert (alone["soft"] != want["soft"]).any(axis=1).sum() >= 28


# ---- the fallbacks, d_primary ----
@pytest.mark.parametrize("sps", [1, 4])
def test_fallbacks_and_primary(sps):
    """A NaN on the non-primary antenna only, a 147-symbol burst and zero energy on both antennas: window word 1, zero taps and the
    oracle's demodulateBurst soft bits of the PRIMARY antenna.  d_enable == 0 and a negative offset on either antenna: window word 2
    and zeros.  d_primary = 1 on an equalised burst: positions 61..86 are antenna 1's demodulator bits, the others do not move."""
    f = dfam.mixed_batch(sps, 2, 9, 6200 + sps)
    o = oraclebind.Oracle(sps)
    B = 9
    x0, x1 = f["x0"].copy(), f["x1"].copy()
    length = f["length"].copy(); off0 = f["off0"].copy(); off1 = f["off1"].copy()
    primary = np.array([0, 0, 1, 1, 0, 1, 0, 0, 1], np.uint8)
    enable = np.ones(B, np.uint8)
    x1[off1[1] + 70 * sps + 1:off1[1] + 71 * sps + 1] = np.complex64(complex(np.nan, 1.0))     # burst 1: NaN on antenna 1, primary 0
    x0[off0[2] + 30 * sps:off0[2] + 31 * sps] = np.complex64(complex(0.0, np.inf))            # burst 2: infinity on antenna 0, primary 1
    length[3] = 147 * sps                                                                     # burst 3: short
    x0[off0[4]:off0[4] + length[4]] = 0; x1[off1[4]:off1[4] + length[4]] = 0                  # burst 4: zero energy on both
    enable[6] = 0                                                                             # burst 6: not enabled
    off1[7] = -1                                                                              # burst 7: antenna 1's offset refused
    got = dm.mlse_div_batch(sps, x0, off0, x1, off1, length, f["tsc"], f["amp"], f["toa"], primary=primary, enable=enable, oracle=o)
    for b in (1, 2, 3, 4):
        assert got["win"][b] == dm.WIN_FELL_BACK and not got["chan"][b].any(), b
        xa, oa = (x1, off1) if primary[b] else (x0, off0)
        with np.errstate(all="ignore"):
            dem = o.demodulate(xa[oa[b]:oa[b] + length[b]], f["amp"][b], f["toa"][b])
        n = min(148, int(length[b]) // sps)
        assert same_nan(got["soft"][b, :n], dem[:n]), b
        assert np.all(got["soft"][b, n:] == 0.5)
    assert np.isfinite(got["soft"][1]).all() and np.isfinite(got["soft"][2]).all()       # the bad antenna was not the primary one
    assert np.all(got["soft"][4] == 0.5)
    for b in (6, 7):
        assert got["win"][b] == dm.WIN_SKIPPED and not got["soft"][b].any() and not got["chan"][b].any()
    for b in (0, 5, 8):
        assert got["win"][b] <= 0 and got["chan"][b, 0].any() and got["chan"][b, 1].any()
        xa, oa = (x1, off1) if primary[b] else (x0, off0)
        dem = o.demodulate(xa[oa[b]:oa[b] + length[b]], f["amp"][b], f["toa"][b])
        assert got["soft"][b, 61:87].tobytes() == dem[61:87].tobytes()
    other = dm.mlse_div_batch(sps, x0, off0, x1, off1, length, f["tsc"], f["amp"], f["toa"], primary=1 - primary, enable=enable, oracle=o)
    for b in (0, 5, 8):
        assert other["soft"][b, mlse_ref.TRELLIS].tobytes() == got["soft"][b, mlse_ref.TRELLIS].tobytes()
        assert other["soft"][b, 61:87].tobytes() != got["soft"][b, 61:87].tobytes()


def test_select_rule():
    """sel = 1 if v_1 && (!v_0 || n_1 > n_0); else 0 if v_0; else 2.  A tie stays with antenna 0, a NaN amplitude compares false
    either way, n is formed in float32 (re*re + im*im, each rounded)."""
    nan = np.complex64(complex(np.nan, 1.0))
    big, small = np.complex64(3 + 4j), np.complex64(1 - 2j)
    rows = [  # v0, amp0, v1, amp1, sel
        (1, small, 1, big, 1), (1, big, 1, small, 0), (1, big, 1, big, 0), (1, np.complex64(5 + 0j), 1, np.complex64(3 - 4j), 0),
        (0, big, 1, small, 1), (1, small, 0, big, 0), (0, big, 0, big, 2), (0, nan, 0, nan, 2),
        (1, nan, 1, big, 0), (1, big, 1, nan, 0), (1, nan, 1, nan, 0), (0, big, 1, nan, 1), (1, nan, 0, big, 0),
        (4, small, 4, big, 1),                                # any non-zero byte is "valid"
    ]
    got = dm.select([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    assert got.dtype == np.uint8 and got.tolist() == [r[4] for r in rows]
    # float32, not float64: the 2^-28 that antenna 1's imaginary part adds is lost beside 1 + 2^-12 -- a tie, antenna 0 stays
    a0 = np.complex64(complex(1.0 + 2.0 ** -13, 0.0)); a1 = np.complex64(complex(1.0 + 2.0 ** -13, 2.0 ** -14))
    assert abs(np.complex128(a1)) ** 2 > abs(np.complex128(a0)) ** 2
    assert dm.select([1], [a0], [1], [a1]).tolist() == [0]


# ---- graded by the float64 reference ----
def graded(sps):
    return dfam.graded_batch(sps, per=24 if sps == 1 else 8)


@pytest.mark.parametrize("sps", [1, 4])
def test_model_within_the_bound(sps):
    """72 bursts at sps 1 (24 at sps 4), independent channels per antenna, clean, 15 dB and 8 dB: no bad_soft, bad_clamp or bad_hard
    anywhere; the payload positions the reference keeps out of the hard-bit comparison are at most 0.5 % per noise level (the
    reference alone decides them).  Measured on the CPU: printed per group."""
    f = graded(sps)
    wt = f["want"]
    eq = wt["win"] <= 0
    assert eq.sum() >= len(eq) - 2 and (sps != 1 or len(eq) >= 64)
    g = dref.check(wt["soft"][eq], wt["hard"][eq], wt["y"][eq], wt["win"][eq], wt["chan"][eq], f["tsc"], "model, sps %d" % sps)
    tally = mlse_ref.Tally(mlse_family.PAYLOAD)
    tally.add(g, f["snr"][eq], f["group"][eq])
    tally.report("two-antenna model (CPU), sps %d" % sps)
    tally.assert_cap("two-antenna model, sps %d" % sps)
    assert set(tally.positions) == {"no noise", "15 dB", "8 dB"}


MUTANTS = {
    "second antenna's metric dropped from gamma": ("g = (dr0 * dr0 + di0 * di0) + (dr1 * dr1 + di1 * di1)", "g = (dr0 * dr0 + di0 * di0)"),
    "E from antenna 0 only": ("p = (c0r * c0r + c0i * c0i) + (c1r * c1r + c1i * c1i)", "p = (c0r * c0r + c0i * c0i)"),
}


def worst_ratio(model, f):
    soft, win, h = model.equalise(f["want"]["y"], f["tsc"], f["primary"])
    eq = win <= 0
    assert eq.sum() >= len(eq) - 2
    g = dref.grade(soft[eq], soft[eq] > 0.5, f["want"]["y"][eq], win[eq], h[eq], f["tsc"])
    return float(g["ratio"].max())


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_is_caught(name):
    """Each mutant exceeds the bound on the graded family (the unmutated copy, built the same way, stays inside)."""
    f = graded(1)
    if name == sorted(MUTANTS)[0]:
        assert worst_ratio(variant(dm), f) <= 1.0
    worst = worst_ratio(variant(dm, MUTANTS[name]), f)
    print("mutant %-44s worst |soft - clamp(soft64)| / bound = %.3g" % (name, worst))
    assert worst > 1.0


# ---- what it is for ----
def test_diversity_pays():
    """sps 4, the "five" profile with independent Rayleigh taps per antenna and burst, a mean SNR of 9 dB with the same noise power on
    both antennas, 60 bursts (seed 31); amplitude and TOA from analyzeTrafficBurst per antenna and select().  Payload bit errors
    (an undetected burst counts as half its bits): the joint equaliser makes strictly fewer than antenna 0 alone and no more than the
    selected antenna alone.  Counted on this CPU, of 6960 payload bits:
        antenna 0 alone 334, selected antenna alone 78, both antennas jointly 64, bursts neither antenna detected 1."""
    r = dfam.rayleigh_family(4, 9.0, 60, 31)
    o, sps, tsc, n = r["o"], r["sps"], r["tsc"], len(r["sel"])
    pay = mlse_family.PAYLOAD
    half = len(pay) // 2
    x0, off0, length = mlse_family.pack(r["xs0"]); x1, off1, _ = mlse_family.pack(r["xs1"])
    one = mm.mlse_batch(sps, x0, off0, length, tsc, r["amp"][:, 0], r["toa"][:, 0], enable=r["v"][:, 0], oracle=o)
    two = mm.mlse_batch(sps, x1, off1, length, tsc, r["amp"][:, 1], r["toa"][:, 1], enable=r["v"][:, 1], oracle=o)
    sel = r["sel"]
    pick = np.where(sel == 1, 1, 0)
    amp = r["amp"][np.arange(n), pick]; toa = r["toa"][np.arange(n), pick]
    joint = dm.mlse_div_batch(sps, x0, off0, x1, off1, length, tsc, amp, toa, primary=pick, enable=(sel < 2), oracle=o)

    def errors(soft, found):
        e = ((soft > 0.5) != r["bits"])[:, pay].sum(axis=1)
        return int(np.where(found, e, half).sum())
    e_one = errors(one["soft"], r["v"][:, 0])
    e_sel = errors(np.where((sel == 1)[:, None], two["soft"], one["soft"]), sel < 2)
    e_joint = errors(joint["soft"], sel < 2)
    print("diversity: antenna 0 alone %d, selected antenna alone %d, jointly %d of %d payload bits; neither detected: %d bursts"
          % (e_one, e_sel, e_joint, n * len(pay), int((sel == 2).sum())))
    assert e_joint < e_one and e_joint <= e_sel
    assert e_one >= 50                                        # the family does fade
