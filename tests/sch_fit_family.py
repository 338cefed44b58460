"""Families for the fit detector's tests (tests/test_sch_fit_model.py, tests/test_gpu_sch_fit.py, tests/test_gpu_l1acq_fit.py):
windows that hold NO synchronisation burst, cut as a search cuts them, with the geometry gate of TRXSIG_SCHDET_FIT applied; and the
measurement of the suggested threshold (include/trxsig_l1acq.h, TRXSIG_L1ACQ_SCH_FIT_THRESH).  Test INPUT generation and
bookkeeping only; the expected values come from tests/sch_fit_model.py.  The SCH-bearing families are tests/mlse_sch_family.py's."""
import functools

import numpy as np

import l1_acq_model as am
import mlse_sch_family as fam
import sch_fit_model as model

F32 = np.float32
NEG_KINDS = ("random", "dummy", "fcch", "alternating")
NEG_PROFILES = ("flat", "five", "precursor")
NEG_SNR_DB = 15.0


@functools.lru_cache(maxsize=None)
def fit_detector(sps, mlse=False):
    return model.FitSchDetector(fam.detector(sps).o, mlse)


def negative_window(rng, o, sps, kind, profile):
    """One window of 172 symbols without an SCH: white noise, or a burst of `kind` 12 +- 4 symbols in, through `profile` at 15 dB."""
    if kind == "noise":
        return (1000.0 * np.sqrt(0.5) * (rng.standard_normal(172 * sps) + 1j * rng.standard_normal(172 * sps))).astype(np.complex64)
    bits = {"random": lambda: rng.integers(0, 2, 148).astype(np.uint8), "dummy": lambda: am.DUMMY.astype(np.uint8),
            "fcch": lambda: np.zeros(148, np.uint8), "alternating": lambda: am.ALTERNATING}[kind]()
    return fam.received(rng, o, bits, sps, profile, NEG_SNR_DB, 12 + int(rng.integers(-4, 5)), 172)


def stream_windows(sps):
    """The stage-2 windows (x, omega) a search cuts out of tests/l1_acq_model.negative_streams (where stage 1 finds an FCCH and the
    window lies inside the stream)."""
    o = fam.detector(sps).o
    out = []
    for name, x in am.negative_streams(o, fam._tx(), sps):
        f = am.fcch_search64(x, sps, 0.5)
        if f["k"] < 0 or not f["found"]:
            continue
        w0, n = am.sch_window(f["k"], sps)
        if w0 >= 0 and w0 + n <= len(x):
            out.append((np.ascontiguousarray(x[w0:w0 + n]), F32(f["omega"])))
    return out


@functools.lru_cache(maxsize=None)
def negative_set(sps, rounds, seed=4100):
    """Set (a): `rounds` windows of each of the 13 classes (white noise; 4 burst kinds x 3 profiles) and the negative streams' SCH
    windows, through the fit detector at threshold +inf: dict(n_windows, n_candidates, q [n_candidates] float32, kind [n_candidates])."""
    rng = np.random.default_rng(seed + sps)
    det = fit_detector(sps)
    o = det.o
    classes = [("noise", None)] + [(k, p) for k in NEG_KINDS for p in NEG_PROFILES]
    q, kinds, n = [], [], 0
    for kind, prof in classes:
        for _ in range(rounds):
            r = det.detect(negative_window(rng, o, sps, kind, prof), None, np.inf)
            n += 1
            if r["candidate"]:
                q.append(r["ptm"]); kinds.append(kind if prof is None else kind + "/" + prof)
    for x, om in stream_windows(sps):
        r = det.detect(x, om, np.inf)
        n += 1
        if r["candidate"]:
            q.append(r["ptm"]); kinds.append("stream")
    return dict(n_windows=n, n_candidates=len(q), q=np.array(q, F32), kind=kinds)


@functools.lru_cache(maxsize=None)
def positive_q(sps, profile, snr_db, n=60, seed=None):
    """q of tests/mlse_sch_family.static_family's n windows under the fit detector (0 for a window that is no candidate), with
    the valley detector's verdict at 8.0 and what that family returns: dict(q [n], candidate [n], valley [n], family)."""
    seed = 5000 + int(snr_db) if seed is None else seed
    f = fam.static_family(sps, profile, snr_db, n, seed)
    det = fit_detector(sps)
    rs = [det.detect(x, None, np.inf) for x in f[4]]
    return dict(q=np.array([r["ptm"] for r in rs], F32), candidate=np.array([r["candidate"] for r in rs], bool), valley=f[7], family=f)
