"""Randomised bit-exact comparison of the CPU oracle against the REAL reference library
(oracle/_ref, built in place from the reference's sources by `make -C oracle ref`).  Where that library
is absent the reference's answers are replayed from tests/golden/ref_calls/ (tests/ref_replay.py)."""
import numpy as np
import pytest

import oraclebind
import refbind
from ref_replay import refs  # noqa: F401  (fixture)
from util import assert_beq


def cn(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def awgn(rng, n, s):
    return (s * cn(rng, n) / np.sqrt(2)).astype(np.complex64)


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_burst_paths(sps, refs):
    rng = np.random.default_rng(1000 + sps)
    o = oraclebind.Oracle(sps); r = refs.sigproc(sps, derive={"modulate": o.modulate, "delay_vector": o.delay_vector})
    tscb, _, rachb = r.gsm_bits()
    for it in range(160):
        tsc = it % 8
        bits = rng.integers(0, 2, 148).astype(np.int8); bits[61:87] = tscb[tsc]
        x = r.modulate(bits, 8 + (it % 4 == 0))
        assert_beq(x, o.modulate(bits, 8 + (it % 4 == 0)), "modulate")
        A = rng.uniform(300, 3000) * np.exp(2j * np.pi * rng.uniform())
        x = r.delay_vector((x * np.complex64(A)).astype(np.complex64), np.float32(rng.uniform(-2.5, 2.5)))
        x = (x + awgn(rng, x.size, (0, 0.1, 0.3, 1.0)[it % 4] * abs(A))).astype(np.complex64)
        ra = r.analyze_traffic(x, tsc, 3.0, req_chan=bool(it & 1)); oa = o.analyze_traffic(x, tsc, 3.0, req_chan=bool(it & 1))
        assert ra["ok"] == oa["ok"] and ra["amp"] == oa["amp"] and ra["toa"] == oa["toa"], (it, ra, oa)
        assert ("chan" in ra) == ("chan" in oa)
        if "chan" in ra:
            assert_beq(ra["chan"], oa["chan"]); assert ra["chan_off"] == oa["chan_off"]
        if ra["amp"] != 0:
            assert_beq(r.demodulate(x, ra["amp"], ra["toa"]), o.demodulate(x, oa["amp"], oa["toa"]), "demod")
        assert r.energy_detect(x, 20 * sps, 100.0) == o.energy_detect(x, 20 * sps, 100.0)
    for it in range(60):
        bits = np.zeros(148, np.int8); bits[:8] = [0, 1, 0, 1, 0, 1, 0, 1]; bits[8:49] = rachb
        bits[49:85] = rng.integers(0, 2, 36)
        x = r.modulate(bits, 8 + (it % 4 == 0))
        A = rng.uniform(300, 3000) * np.exp(2j * np.pi * rng.uniform())
        x = r.delay_vector((x * np.complex64(A)).astype(np.complex64), np.float32(rng.integers(0, 61) * sps + rng.uniform()))
        x = (x + awgn(rng, x.size, (0, 0.1, 0.3, 2.0)[it % 4] * abs(A))).astype(np.complex64)
        rr = r.detect_rach(x); ro = o.detect_rach(x)
        assert rr["ok"] == ro["ok"] and rr["amp"] == ro["amp"] and rr["toa"] == ro["toa"], (it, rr, ro)
        if rr["amp"] != 0:
            assert_beq(r.demodulate(x, rr["amp"], rr["toa"]), o.demodulate(x, ro["amp"], ro["toa"]), "demod")


def test_primitives_random(refs):
    rng = np.random.default_rng(2000)
    o = oraclebind.Oracle(4); r = refs.sigproc(4, derive={"delay_vector": o.delay_vector})
    for span in range(5):
        for (ar, br) in [(0, 0), (1, 0), (0, 1), (1, 1)]:
            for (na, nb) in [(50, 7), (50, 8), (7, 50), (30, 30), (1, 1), (5, 1)]:
                a = cn(rng, na); b = cn(rng, nb)
                if ar: a = a.real.astype(np.complex64)
                if br: b = b.real.astype(np.complex64)
                assert_beq(r.convolve(a, b, span, ar, br), o.convolve(a, b, span, ar, br))
                assert_beq(r.correlate(a, b, span, ar, br), o.correlate(a, b, span, ar, br))
    for it in range(200):
        n = int(rng.integers(5, 700)); x = cn(rng, n); d = np.float32(rng.uniform(-8, 8))
        if it % 10 == 0: d = np.float32(np.round(d))
        if it % 10 == 1: d = np.float32(np.round(d) + 0.005)
        assert_beq(r.delay_vector(x, d), o.delay_vector(x, d))
        ix = np.float32(rng.uniform(-3, n + 3))
        assert r.interpolate_point(x, ix) == o.interpolate_point(x, ix)
        assert r.peak_detect(x) == o.peak_detect(x)
    xs = rng.uniform(-60, 60, 3000).astype(np.float32)
    for x in xs:
        assert r.sinc(x) == o.sinc(x) and r.sinLookup(x) == o.sinLookup(x) and r.cosLookup(x) == o.cosLookup(x)


def test_resample_random(refs):
    rng = np.random.default_rng(3000)
    r = refs.sigproc(4); o = oraclebind.Oracle(4)
    rcv, snd = r.lpf_raw()
    snd961 = np.concatenate([snd, [0]]).astype(np.float32)
    assert_beq(r.create_lpf651(260.0), o.create_lpf(rcv, 260.0))
    lrx = o.create_lpf(snd961, 260.0); ltx = o.create_lpf(rcv, 96.0)
    for (n, P, Q, l) in [(1056, 260, 96, lrx), (1056, 260, 96, o.create_lpf(rcv, 260.0)), (3000, 96, 260, ltx),
                         (300, 65, 96, ltx), (100, 3, 2, ltx[:101].copy()), (17, 260, 96, lrx)]:
        x = cn(rng, n)
        assert_beq(r.polyphase_resample(x, P, Q, l), o.polyphase_resample(x, P, Q, l), "resample %d %d %d" % (n, P, Q))


@pytest.mark.parametrize("variant", ["", "52m"])
def test_dfe_flow(variant, refs):
    rng = np.random.default_rng(4000)
    o = oraclebind.Oracle(1, variant52m=(variant == "52m"))
    r = refs.sigproc(1, variant, derive={"modulate": o.modulate, "delay_vector": o.delay_vector, "convolve": o.convolve,
                                         "scale_vector": o.scale_vector})
    for t in range(8):
        sq, toa, g = r.midamble(t)
        assert_beq(sq, o.mid[t]); assert np.float32(toa) == o.mid_toa[t] and np.complex64(g) == o.mid_gain[t]
    tscb, _, _ = r.gsm_bits()
    for it in range(150):
        tsc = it % 8
        bits = rng.integers(0, 2, 148).astype(np.int8); bits[61:87] = tscb[tsc]
        x = r.modulate(bits, 8 + (it % 4 == 0))
        A = rng.uniform(300, 2000) * np.exp(2j * np.pi * rng.uniform())
        x = r.delay_vector((x * np.complex64(A)).astype(np.complex64), np.float32(rng.uniform(-1.5, 1.5)))
        ch = np.array([1, 0.4 + 0.2j, 0], np.complex64) if it % 2 else np.array([1, 0, 0.3j], np.complex64)
        x = r.convolve(x, ch, refbind.START_ONLY)
        x = (x + awgn(rng, x.size, (0.02, 0.1, 0.2)[it % 3] * abs(A))).astype(np.complex64)
        mt = (0, 4, 6)[it % 3]
        ra = r.analyze_traffic(x, tsc, 3.0, req_chan=True, max_toa=mt)
        oa = o.analyze_traffic(x, tsc, 3.0, req_chan=True, max_toa=mt)
        assert ra["ok"] == oa["ok"] and ra["amp"] == oa["amp"] and ra["toa"] == oa["toa"], (it, ra, oa)
        assert r.energy_detect(x, 20, 5.0) == o.energy_detect(x, 20, 5.0)
        if "chan" in ra:
            assert_beq(ra["chan"], oa["chan"]); assert ra["chan_off"] == oa["chan_off"]
            inv = 1 / complex(ra["amp"])
            chn = r.scale_vector(ra["chan"], inv)
            assert_beq(chn, o.scale_vector(ra["chan"], inv))
            snr = float(abs(ra["amp"]) ** 2 / 101.0)
            d1 = r.design_dfe(chn, snr, 7); d2 = o.design_dfe(chn, snr, 7)
            assert_beq(d1[0], d2[0]); assert_beq(d1[1], d2[1])
            xs = r.scale_vector(x, inv)
            t = np.float32(ra["toa"] - ra["chan_off"])
            assert_beq(r.equalize(xs, t, d1[0], d1[1]), o.equalize(xs, t, d1[0], d1[1]), "equalize")


@pytest.mark.parametrize("variant", ["", "52m"])
def test_equalised_leg_strung_together_inside_the_reference(variant, refs):
    """oracle/ref_driver.cpp::ref_eq_batch runs energyDetect -> analyzeTrafficBurst(requestChannel) -> SNR, scaleVector, designDFE
    -> scaleVector, equalizeBurst(TOA - chanRespOffset) burst by burst INSIDE the compiled reference, as Transceiver::pullRadioVector
    strings them together (Transceiver.cpp:298, 331-349, 391-396) -- bench.py's config-5 cpu_baseline times it.  The oracle's chain
    of the same calls (what the GPU parity tests compare with) gives the same verdicts and the same soft bits."""
    import _pkg
    _pkg.load()
    from openbts_ttsou_amd import synth
    B, tsc, thr = 384, 6, 10.0
    x, off, length, meta = synth.normal_batch(1, B, tsc, seed=55, sigmas=(0.02, 0.1, 0.4), max_delay=1.0)
    for i in range(1, B, 2):                                            # a two-path channel on every other burst
        s = x[off[i]:off[i] + length[i]]
        s[1:] = s[1:] + np.complex64(0.4 + 0.2j) * s[:-1].copy()
    for i in range(0, B, 16):                                           # and some below the energy gate
        x[off[i]:off[i] + length[i]] *= np.float32(1e-3)
    r = refs.sigproc(1, variant); o = oraclebind.Oracle(1, variant52m=(variant == "52m"))
    ok, soft = r.eq_batch(x, off, length, tsc, 3.0, thr, 4)
    n_ok = 0
    for i in range(B):
        s = x[off[i]:off[i] + length[i]]
        ok_e, _ = o.energy_detect(s, 20, thr)
        sv = None
        if ok_e:
            a = o.analyze_traffic(s, tsc, 3.0, req_chan=True, max_toa=4)
            if a["ok"]:
                am = a["amp"]
                n2 = np.float32(np.float32(am.imag * am.imag) + np.float32(am.real * am.real))
                inv = complex(np.float32(am.real / n2), np.float32(-am.imag / n2))
                snr = np.float32(np.float64(n2) / (np.float64(np.float32(thr * thr)) + 1.0))
                w, b = o.design_dfe(o.scale_vector(a["chan"], inv), float(snr), 7)
                sv = o.equalize(o.scale_vector(s, inv), np.float32(a["toa"] - a["chan_off"]), w, b)
        assert (sv is not None) == bool(ok[i]), i
        if sv is not None:
            n_ok += 1
            assert np.array_equal(sv[:156], soft[i, :len(sv)][:156]), i
        else:
            assert not soft[i].any()
    assert 200 < n_ok < B
