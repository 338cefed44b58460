"""The CPU model of mobile-side acquisition (tests/l1_acq_model.py) on its own -- no GPU.  On the very streams the GPU test uses
the model finds every FCCH, estimates the offset, detects, demodulates and decodes the SCH behind it and places the frame grid;
the negative families stay negative; and a float32 emulation shows why the header demands segment scans: they stay within the
tolerance beside a slot 40 dB up, where one differenced running sum does not."""
import numpy as np
import pytest

import fectxbind
import l1_acq_model as am
import oraclebind


@pytest.fixture(scope="module")
def tx():
    return fectxbind.FecTxOracle()


@pytest.fixture(scope="module", params=[1, 4])
def det(request):
    return am.SchDetector(oraclebind.Oracle(request.param))


def test_sequence(det):
    sps = det.sps
    assert det.seq.shape == (64 * sps,) and abs(det.gain) > 10 * sps
    # the autocorrelation peaks where a NO_DELAY correlation puts lag zero: the middle of the vector
    assert abs(float(det.toa) - 32 * sps) <= 1.0


def test_truth(det, tx):
    sps, o = det.sps, det.o
    worst_t = worst_f = 0.0
    for case in am.truth_cases(sps):
        x, sch = am.truth_stream(o, tx, case)
        r = am.search_model(det, tx, x)
        assert r["state"] == 15, (case, r["state"])
        at = r["w0"] + float(r["sch"]["toa"])
        fn, true = min(sch, key=lambda s: abs(s[1] - at))
        assert (r["bsic"], r["rfn"]) == (case["bsic"], fn), case
        worst_t = max(worst_t, abs(at - true))
        worst_f = max(worst_f, abs(r["fcch"]["arg"] / (2 * np.pi) - case["f"]))
        assert r["sch"]["ptm"] > 14
    print("sps %d: worst timing error %.3f sample, worst frequency error %.2e cycle / symbol" % (sps, worst_t, worst_f))
    assert worst_t <= 0.25 and worst_f <= 2e-3


def test_negative_families(det, tx):
    sps = det.sps
    for name, x in am.negative_streams(det.o, tx, sps):
        r = am.search_model(det, tx, x)
        if name == "no_fcch":
            assert r["state"] == 0 and r["fcch"]["m"] < 0.5, (name, r["fcch"]["m"])
        elif name == "no_sch":
            assert r["state"] == 3 and r["sch"]["ptm"] <= 8.0, (name, r["state"], r["sch"] and r["sch"]["ptm"])
        else:
            assert r["state"] == 1, (name, r["state"])


def test_segment_scans_hold_beside_a_loud_slot(det, tx):
    sps = det.sps
    rng = np.random.default_rng(5)
    clean, _ = am.build_stream(det.o, tx, rng, 0, 3, 9, loud=100.0)
    x = am.impair(clean, rng, sps, 0, 2, 0.02, 1.0, None)
    m64 = am.fcch_metric64(x, sps)[2]
    seg = am.fcch_metric32_segments(x, sps)
    run = am.fcch_metric32_segments(x, sps, running=True)
    assert np.abs(seg - m64).max() <= am.fcch_tol(sps)
    k = int(np.argmax(m64))
    assert m64[k] > 0.9 and abs(seg[k] - m64[k]) <= am.fcch_tol(sps)
    assert np.abs(run - m64).max() > 10 * am.fcch_tol(sps)    # the differenced running sum loses the quiet burst


def test_short_and_poisoned_streams():
    C, E, m = am.fcch_metric64(np.ones(142 + 1 - 1, np.complex64), 1)
    assert len(m) == 0 and am.fcch_search64(np.ones(100, np.complex64), 1)["k"] == -1
    x = np.exp(0.5j * np.pi * np.arange(600)).astype(np.complex64)
    x[300] = np.nan
    x[310] = np.inf
    m = am.fcch_metric64(x, 1)[2]
    assert (m[300 - 142:311] == 0).all() and m[:150].min() > 0.999 and m[312:].min() > 0.999
