"""Proof, on the CPU, that the equaliser family of tests/eq_family.py is what it claims: the oracle is the real reference on
every member (live where oracle/_ref is built, replayed from tests/golden/ref_calls/ elsewhere; results that may hold a NaN
are recorded in full and compared position by position, everything else bit for bit through digests), the zero-pad mutant
and the geometry mutant are seen by the members meant to catch them and by no others, and the conditions that keep
tests/test_gpu_eq_family.py honest hold."""
import numpy as np
import pytest

import eq_family as ef
import oraclebind
from ref_replay import refs  # noqa: F401  (fixture)
from util import assert_beq, assert_veq_nan


@pytest.fixture(autouse=True)
def quiet_floats():
    with np.errstate(all="ignore"):                            # the members overflow and divide by zero on purpose
        yield


@pytest.fixture(scope="module")
def oracles():
    return {False: oraclebind.Oracle(1), True: oraclebind.Oracle(1, variant52m=True)}


def reported(o):
    """o.analyze_traffic without the oracle's extra (peak_to_mean): what the reference's binding returns."""
    def call(*a, **kw):
        r = o.analyze_traffic(*a, **kw)
        r.pop("peak_to_mean")
        return r
    return call


def same_analysis(ra, oa, what):
    assert ra["ok"] == oa["ok"], what
    assert_veq_nan(ra["amp"], oa["amp"], what); assert_veq_nan(ra["toa"], oa["toa"], what)
    assert ("chan" in ra) == (oa.get("chan") is not None), what
    if "chan" in ra:
        assert_veq_nan(ra["chan"], oa["chan"], what); assert ra["chan_off"] == oa["chan_off"], what


# ---- the oracle is the reference ----
def test_oracle_is_the_reference_geometry(oracles, refs):
    """Every member at every maxTOA through the 52M reference's analyzeTrafficBurst, and each maxTOA's batch through the
    whole leg inside the reference (ref_eq_batch, energy gate at 10)."""
    o = oracles[True]
    r = refs.sigproc(1, "52m", derive={"analyze_traffic": reported(o), "eq_batch": lambda *a: ef.chain_batch(o, *a)})
    for mt in ef.MAX_TOAS:
        g = ef.geometry(mt)
        for i in range(len(g)):
            ra = r.analyze_traffic(g.burst(i), g.tsc, 3.0, req_chan=True, max_toa=mt)
            oa = o.analyze_traffic(g.burst(i), g.tsc, 3.0, req_chan=True, max_toa=mt)
            assert ra["ok"] == oa["ok"] and ra["amp"] == oa["amp"] and ra["toa"] == oa["toa"], (mt, i, ra, oa)
            if "chan" in ra:
                assert_beq(ra["chan"], oa["chan"]); assert ra["chan_off"] == oa["chan_off"]
        ok, soft = r.eq_batch(g.x, g.off, g.length, g.tsc, 3.0, 10.0, mt)
        wok, wsoft = ef.chain_batch(o, g.x, g.off, g.length, g.tsc, 3.0, 10.0, mt)
        assert np.array_equal(ok, wok) and ok.sum() > len(g) // 4, mt
        assert_beq(soft, wsoft, "maxTOA %d" % mt)


@pytest.mark.parametrize("variant", ["", "52m"])
def test_oracle_is_the_reference_channels(oracles, refs, variant):
    o = oracles[variant == "52m"]
    r = refs.sigproc(1, variant)
    c = ef.channels()
    for i in range(len(c)):
        h = c.scaled(o, i)
        (rw, rb), (ow, ob) = r.design_dfe(h, float(c.snr[i]), 7), o.design_dfe(h, float(c.snr[i]), 7)
        assert_veq_nan(rw, ow, c.name[i]); assert_veq_nan(rb, ob, c.name[i])


@pytest.mark.parametrize("variant", ["", "52m"])
def test_oracle_is_the_reference_bursts(oracles, refs, variant):
    """analyzeTrafficBurst member by member; the finite members through the whole leg inside the reference, with the
    energy gate at 10 and at 0 (which lets every detected rung of the ladder through to designDFE and equalizeBurst: at
    least 75 of 84, the regime where 1 / sqrt(SNR) swamps the channel included); the members with a non-finite sample call
    by call (their soft bits hold NaNs, whose payloads the two do not share)."""
    v52 = variant == "52m"
    o = oracles[v52]
    rd = refs.sigproc(1, variant, derive={"eq_batch": lambda *a: ef.chain_batch(o, *a)})
    r = refs.sigproc(1, variant)
    bt = ef.bursts()
    for i in range(len(bt)):
        ra = r.analyze_traffic(bt.burst(i), bt.tsc, 3.0, req_chan=True, max_toa=bt.max_toa)
        c = ef.oracle_chain(o, bt.burst(i), bt.tsc, 10.0, v52, bt.max_toa)
        same_analysis(ra, c, (variant, i, bt.cls[i]))
        if not (bt.hostile[i] and c["ok"]):
            continue
        inv = ef.inv_amp(c["amp"])
        rw, rb = r.design_dfe(o.scale_vector(c["chan"], inv), float(c["snr"]), 7)
        assert_veq_nan(rw, c["w"], i); assert_veq_nan(rb, c["b"], i)
        assert_veq_nan(r.equalize(o.scale_vector(bt.burst(i), inv), np.float32(c["toa"] - c["chan_off"]), c["w"], c["b"]), c["soft"], i)
    keep = np.flatnonzero(~bt.hostile)
    f = bt.take(keep)
    ladder = bt.cls[keep] == "ladder"
    for thr, rungs in ((10.0, 55), (0.0, 75)):                  # a gate at 10 refuses the rungs below 2^-7; at 0 every detected rung passes
        ok, soft = rd.eq_batch(f.x, f.off, f.length, bt.tsc, 3.0, thr, bt.max_toa)
        wok, wsoft = ef.chain_batch(o, f.x, f.off, f.length, bt.tsc, 3.0, thr, bt.max_toa)
        assert np.array_equal(ok, wok) and rungs <= ok[ladder].sum() < rungs + 9, (thr, ok[ladder].sum())
        assert_beq(soft, wsoft)


def test_oracle_is_the_reference_taps(oracles, refs):
    """(equalizeBurst is the same text in both variants: the Transceiver/ library serves.)"""
    o = oracles[False]
    rd = refs.sigproc(1, "", derive={"equalize": o.equalize})
    r = refs.sigproc(1, "")
    t = ef.taps()
    for i in range(len(t)):
        s = o.scale_vector(t.burst(i), ef.inv_amp(t.amp[i]))
        want = o.equalize(s, t.toa[i], t.w[i], t.b[i])
        if np.isfinite(want).all():
            assert_beq(rd.equalize(s, t.toa[i], t.w[i], t.b[i]), want, "member %d" % i)
        else:
            assert_veq_nan(r.equalize(s, t.toa[i], t.w[i], t.b[i]), want, "member %d (%s)" % (i, t.cls[i]))


# ---- the family bites ----
def test_zero_pad_mutant(oracles):
    """equalizeBurst of the burst followed by six zero samples, cut back to the burst: what an equaliser computes that adds
    the product with a zero sample where the reference skips the term.  With w[j] not finite the reference's last 6 - j
    soft bits are finite and the mutant's are NaN (j = 6 is never skipped: 6 of the 42 members cannot tell); with finite taps
    the two are the same values."""
    o = oracles[False]
    t = ef.taps()
    seen = {"w": [0, 0], "finite": [0, 0]}
    for i in np.flatnonzero(t.at0 & np.isin(t.cls, ("w", "finite"))):
        good, bad = ef.equalize_member(o, t, i), ef.equalize_member(o, t, i, pad=6)
        differs = not ef.same_with_nan(good, bad)
        seen[t.cls[i]][0] += 1; seen[t.cls[i]][1] += differs
        if t.cls[i] == "w":
            (j, vi, part), n = t.bad[i], int(t.length[i])
            assert not np.isnan(good[n - 6 + j:]).any() and np.isnan(bad[n - 6 + j:]).all(), (i, j)    # 0 * Inf is a NaN too
            if np.isnan(ef.BAD[vi]):                           # (an Inf tap gives Inf or NaN before the slicer: 0, 1 or NaN after it)
                assert np.isnan(good[:n - 6 + j]).all() and np.isnan(bad).all(), (i, j)
            assert differs == (j < 6), (i, j)
    print("zero-pad mutant: %d of %d one-bad-component w members, %d of %d finite-tap members" % (
        seen["w"][1], seen["w"][0], seen["finite"][1], seen["finite"][0]))
    assert seen["w"][0] == 42 and seen["w"][1] >= 0.75 * seen["w"][0]
    assert seen["finite"][0] == 66 and seen["finite"][1] == 0


def test_geometry_mutant(oracles):
    """The oracle asked with maxTOA - 1: the window's first lag, its length and the TOA's origin move, so amplitude or TOA
    of EVERY detected member changes -- for maxTOA >= 4.  Below, maxTOA is clamped to 3 and nothing may change."""
    o = oracles[True]
    for mt in ef.MAX_TOAS[1:]:
        g = ef.geometry(mt)
        ndet = nchanged = 0
        for i in range(len(g)):
            a = o.analyze_traffic(g.burst(i), g.tsc, 3.0, req_chan=True, max_toa=mt)
            m = o.analyze_traffic(g.burst(i), g.tsc, 3.0, req_chan=True, max_toa=mt - 1)
            changed = not (a["ok"] == m["ok"] and a["amp"] == m["amp"] and a["toa"] == m["toa"])
            if mt <= 3:
                assert not changed and np.array_equal(a.get("chan"), m.get("chan")), (mt, i)
            elif a["ok"]:
                ndet += 1; nchanged += changed
        if mt >= 4:
            print("maxTOA %2d: the mutant changes %d of %d detected members" % (mt, nchanged, ndet))
            assert nchanged == ndet > len(g) // 4, (mt, nchanged, ndet)


# ---- conditions that keep the GPU test honest ----
def test_geometry_members_are_detected_on_many_lags(oracles):
    o = oracles[True]
    for mt in ef.MAX_TOAS:
        for integers in (False, True) if mt in ef.FP16_MAX_TOAS else (False,):
            g = ef.geometry(mt, integers)
            assert len(g) % 64 and set(g.kind) == {-1, 0, 1, 2, 3} and g.length.min() >= ef.ragged_floor(mt) and (g.length < 156).any()
            res = [o.analyze_traffic(g.burst(i), g.tsc, 3.0, req_chan=True, max_toa=mt) for i in range(len(g))]
            ndet = sum(a["ok"] for a in res)
            lags = {int(np.rint(a["toa"])) for a in res if a["ok"]}
            print("maxTOA %2d%s: %d of %d detected on %d lags" % (mt, " (integers)" if integers else "", ndet, len(g), len(lags)))
            assert ndet >= len(g) / 4 and len(lags) >= 4, (mt, ndet, sorted(lags))
            if integers:
                h = g.x.view(np.float32)
                assert np.array_equal(h, h.astype(np.float16).astype(np.float32)) and np.abs(h).max() <= 2048
    assert len({ef.geometry(mt).tsc for mt in ef.MAX_TOAS}) == 8


def test_channels_are_mostly_finite(oracles):
    o = oracles[False]
    c = ef.channels()
    finite = 0
    for i in range(len(c)):
        w, b = o.design_dfe(c.scaled(o, i), float(c.snr[i]), 7)
        finite += bool(np.isfinite(w.view(np.float32)).all() and np.isfinite(b.view(np.float32)).all())
    print("%d of %d channel cases give all-finite taps" % (finite, len(c)))
    assert finite >= 40 and len(c) - finite >= 5
    assert c.use_amp.sum() >= 8 and {0.0, np.inf} <= set(np.abs(c.amp[c.use_amp]).tolist()) and np.isnan(c.amp).any()
    assert set(np.float32(ef.SNRS)[:-1].tolist()) <= set(c.snr.tolist()) and np.isnan(c.snr).any()


@pytest.mark.parametrize("v52", [False, True], ids=["transceiver", "52m"])
def test_ladder_is_detected_and_finite(oracles, v52):
    o = oracles[v52]
    bt = ef.bursts()
    ladder = np.flatnonzero(bt.cls == "ladder")
    assert len(ladder) == len(bt.ladder_k) == 84
    det = []
    for i, k in zip(ladder, bt.ladder_k):
        c = ef.oracle_chain(o, bt.burst(i), bt.tsc, 10.0, v52, bt.max_toa)
        if c["ok"]:
            det.append(k)
            for key in ("amp", "toa", "chan", "w", "b", "soft"):
                assert np.isfinite(c[key]).all(), (k, key)
    print("ladder detected for 2^%d .. 2^%d" % (det[0], det[-1]))
    assert det == list(range(det[0], det[-1] + 1)) and det[0] <= -27 and det[-1] >= 50 and len(det) < 84   # both ends fail
    assert bt.hostile.sum() == 12 and len(bt) % 64
    for cls in ("echoes", "null", "maxphase", "constant", "plain"):
        assert (bt.cls == cls).any()
