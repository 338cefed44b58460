"""Acquisition's fit detector on the GPU (trxsig_l1acq_set_sch_detector, trxsig_l1acq_sch_fit; include/trxsig_l1acq.h), at sps 1
and 4.

  detect_sch_batch   under FIT, on 9 windows of each static profile at 15 dB, 9 windows without an SCH and one of length 0: flags,
                     amp, toa, q (in d_ptm), soft and hard bits equal tests/sch_fit_model.py's FitSchDetector on both legs
  VALLEY             after the setter has been used and set back, search and detect_sch_batch give a fresh object's outputs byte
                     for byte, and trxsig_l1acq_sch_fit hands out zeros
  a search           tests/mlse_sch_family.search_streams (three symbols of spread, 12 dB) at the DEFAULT thresholds: on FIT + MLSE
                     d_state, d_rfn, d_bsic and the rest equal l1_acq_model.search_model with the fit detector (fed with the
                     library's window and shift) -- state 15 with the right FN and BSIC on all four; on VALLEY they equal the
                     valley model's prediction: state 3 on all four
  negative streams   tests/l1_acq_model.negative_streams reach no state bit 4 under FIT"""
import numpy as np
import pytest

import _pkg
import l1_acq_model as am
import mlse_sch_family as family
import sch_fit_family as ff

pytestmark = pytest.mark.gpu
EINVAL = -1
FIT_THRESH, VALLEY_THRESH = 1.4, 8.0
KEYS = ("state", "fcch_k", "fcch_metric", "fcch_c", "fcch_e", "arg", "omega", "sch_w0", "sch_ptm", "sch_amp", "sch_toa", "soft", "ok", "bsic", "rfn")


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Rig:
    def __init__(self, pkg, sps):
        self.pkg, self.sps = pkg, sps
        self.ctx = pkg.TrxSig(sps, 0)
        self.ctx.use_torch_stream()
        self.tx = family._tx()
        self.o = family.detector(sps).o
        self.streams = family.search_streams(sps)
        N = len(self.streams[0][0])
        self.N, self.stride = N, N + 3
        buf = np.zeros((len(self.streams), self.stride), np.complex64)
        for i, (x, _) in enumerate(self.streams):
            buf[i, :N] = x
        self.d = dev(buf.ravel().view(np.float32))
        # the windows of detect_sch_batch: 9 of each profile, 9 without an SCH, one of length 0
        rng = np.random.default_rng(8800 + sps)
        xs = []
        for p in ("flat", "five", "precursor"):
            xs += family.static_family(sps, p, 15.0, 9, 8810 + sps)[4]
        kinds = [("noise", None), ("random", "flat"), ("random", "five"), ("random", "precursor"), ("dummy", "five"), ("dummy", "precursor"),
                 ("fcch", "five"), ("alternating", "five"), ("random", "five")]
        cand, rest, det = [], [], ff.fit_detector(sps)          # 5 that pass the geometry gate (about one in ten does) and 4 that do not
        for i in range(400):
            if len(cand) >= 5 and len(rest) >= 4:
                break
            x = ff.negative_window(rng, self.o, sps, *kinds[i % len(kinds)])
            (cand if det.detect(x, None, np.inf)["candidate"] else rest).append(x)
        xs += cand[:5] + rest[:4]
        assert len(xs) == 36
        self.wx = xs
        self.woff = np.r_[np.cumsum([0] + [len(x) + 5 for x in xs])[:-1], 7].astype(np.int32)
        self.wlen = np.r_[[len(x) for x in xs], 0].astype(np.int32)
        flat = np.zeros(int(self.woff[-2] + self.wlen[-2] + 8), np.complex64)
        for o_, x in zip(self.woff, xs):
            flat[o_:o_ + len(x)] = x
        self.dw = dev(flat.view(np.float32))

    def search(self, acq, sch_thresh):
        acq.search(self.d, self.stride, self.N, len(self.streams), 0.5, sch_thresh)
        return acq.collect()

    def detect(self, acq, thresh, with_ptm=True):
        import torch
        B = len(self.woff)
        flags, amp, toa, ptm = (torch.full((B,), 77, dtype=torch.uint8).cuda(), torch.ones(B, 2).cuda(), torch.ones(B).cuda(), torch.ones(B).cuda())
        soft, hard = torch.full((B, 150), -1.0).cuda(), torch.full((B, 150), 255, dtype=torch.uint8).cuda()
        acq.detect_sch(self.dw, dev(self.woff), dev(self.wlen), flags, amp, toa, soft, ptm=ptm if with_ptm else None, hard=hard, detect_thresh=thresh)
        self.ctx.synchronize()
        return dict(flags=flags.cpu().numpy(), amp=amp.cpu().numpy().view(np.complex64).ravel(), toa=toa.cpu().numpy(), ptm=ptm.cpu().numpy(),
                    soft=soft.cpu().numpy(), hard=hard.cpu().numpy())


@pytest.fixture(scope="module", params=[1, 4])
def rig(request, pkg):
    return Rig(pkg, request.param)


@pytest.fixture(scope="module")
def runs(rig):
    """One search and one detect_sch_batch per setting, shared: a fresh object on VALLEY; one object on FIT + DEMOD, FIT + MLSE, and
    set back to VALLEY + DEMOD."""
    pkg = rig.pkg
    S = len(rig.streams)
    fresh = pkg.L1Acq(rig.ctx, S, rig.N)
    out = dict(fresh_search=rig.search(fresh, VALLEY_THRESH), fresh_detect=rig.detect(fresh, VALLEY_THRESH), fresh_fit=fresh.sch_fit())
    fresh.destroy()
    acq = pkg.L1Acq(rig.ctx, S, rig.N)
    acq.set_sch_detector(pkg.SCHDET_FIT)
    out["fit_demod_detect"] = rig.detect(acq, FIT_THRESH)
    out["fit_demod_detect_no_ptm"] = rig.detect(acq, FIT_THRESH, with_ptm=False)
    out["fit_demod_search"] = rig.search(acq, FIT_THRESH)
    acq.set_sch_leg(pkg.SCHLEG_MLSE)
    out["fit_mlse_search"] = rig.search(acq, FIT_THRESH)
    out["fit_mlse_fit"] = acq.sch_fit()
    out["fit_mlse_channel"] = acq.sch_channel()
    out["fit_mlse_detect"] = rig.detect(acq, FIT_THRESH)
    out["fit_mlse_fit_after_detect"] = acq.sch_fit()
    acq.set_sch_detector(pkg.SCHDET_VALLEY)
    out["valley_mlse_search"] = rig.search(acq, VALLEY_THRESH)
    acq.set_sch_leg(pkg.SCHLEG_DEMOD)
    out["back_search"] = rig.search(acq, VALLEY_THRESH)
    out["back_detect"] = rig.detect(acq, VALLEY_THRESH)
    out["back_fit"] = acq.sch_fit()
    acq.destroy()
    return out


def test_valley_is_unchanged_by_a_byte(rig, runs):
    for k in KEYS:
        assert runs["back_search"][k].tobytes() == runs["fresh_search"][k].tobytes(), "search: " + k
    for k in runs["fresh_detect"]:
        assert runs["back_detect"][k].tobytes() == runs["fresh_detect"][k].tobytes(), "detect_sch_batch: " + k
    for name in ("fresh_fit", "back_fit"):
        q, R = runs[name]
        assert q.shape == R.shape == (len(rig.streams),) and not q.any() and not R.any(), name


def test_detect_sch_batch_under_fit(rig, runs):
    """Both legs against the model, window by window; flags, amp, toa and q do not depend on the leg; d_ptm may be NULL; nothing
    is written past 148 values; the accessor still shows the last SEARCH."""
    sps = rig.sps
    d, m = runs["fit_demod_detect"], runs["fit_mlse_detect"]
    for k in ("flags", "amp", "toa", "ptm"):
        assert m[k].tobytes() == d[k].tobytes(), k
    n = runs["fit_demod_detect_no_ptm"]
    assert (n["ptm"] == 1.0).all()
    for k in ("flags", "amp", "toa", "soft", "hard"):
        assert n[k].tobytes() == d[k].tobytes(), "without d_ptm: " + k
    seen = {"pos": 0, "neg_candidates": 0}
    for leg, g, det in (("DEMOD", d, ff.fit_detector(sps)), ("MLSE", m, ff.fit_detector(sps, True))):
        for b, x in enumerate(rig.wx):
            want = det.detect(x, None, FIT_THRESH)
            what = "sps %d %s window %d" % (sps, leg, b)
            assert g["flags"][b] == want["flags"] and g["amp"][b] == want["amp"] and g["toa"][b] == want["toa"] and g["ptm"][b] == want["ptm"], \
                (what, g["flags"][b], want["flags"], g["ptm"][b], want["ptm"])
            assert np.array_equal(g["soft"][b, :148], want["soft"]), (what, np.abs(g["soft"][b, :148] - want["soft"]).max())
            assert np.array_equal(g["hard"][b, :148], (want["soft"] > 0.5).astype(np.uint8)), what
            if leg == "DEMOD":
                seen["pos"] += int(b < 27 and want["flags"] == 2)
                seen["neg_candidates"] += int(b >= 27 and want["candidate"])
                assert b < 27 or want["flags"] == 0, what
        last = len(rig.wx)
        assert g["flags"][last] == 128 and g["amp"][last] == 0 and g["toa"][last] == 0 and g["ptm"][last] == 0 and not g["soft"][last, :148].any()
        assert (g["soft"][:, 148:] == -1).all() and (g["hard"][:, 148:] == 255).all()
    print("sps %d: %d of 27 SCH windows detected, %d of 9 others are candidates" % (sps, seen["pos"], seen["neg_candidates"]))
    assert seen["pos"] == 27 and seen["neg_candidates"] == 5
    assert not np.array_equal(m["soft"][9:27, :148], d["soft"][9:27, :148])       # (the legs do differ on the multipath windows)
    for a, b in zip(runs["fit_mlse_fit"], runs["fit_mlse_fit_after_detect"]):
        assert a.tobytes() == b.tobytes()


def test_search_at_the_default_thresholds(rig, runs):
    sps = rig.sps
    gv, gvm, gfd, gfm = runs["fresh_search"], runs["valley_mlse_search"], runs["fit_demod_search"], runs["fit_mlse_search"]
    for g in (gvm, gfd, gfm):
        for k in ("fcch_k", "fcch_metric", "fcch_c", "fcch_e", "arg", "omega", "sch_w0", "sch_toa"):
            assert g[k].tobytes() == gv[k].tobytes(), k
    for k in ("sch_ptm", "sch_amp", "sch_toa"):
        assert gfm[k].tobytes() == gfd[k].tobytes(), k
    assert np.array_equal(gfm["state"] & 7, gfd["state"] & 7)
    q, R = runs["fit_mlse_fit"]
    chan, win = runs["fit_mlse_channel"]
    n15 = {}
    for name, g, det, th in (("VALLEY + DEMOD", gv, family.detector(sps), VALLEY_THRESH),
                             ("VALLEY + MLSE", gvm, family.MlseSchDetector(rig.o), VALLEY_THRESH),
                             ("FIT + DEMOD", gfd, ff.fit_detector(sps), FIT_THRESH), ("FIT + MLSE", gfm, ff.fit_detector(sps, True), FIT_THRESH)):
        n15[name] = 0
        for i, (x, case) in enumerate(rig.streams):
            what = "sps %d %s stream %d" % (sps, name, i)
            r = am.search_model(det, rig.tx, x, 0.5, th, k=int(g["fcch_k"][i]), omega=g["omega"][i])
            assert int(g["state"][i]) == r["state"], (what, int(g["state"][i]), r["state"])
            s = r["sch"]
            assert int(g["sch_w0"][i]) == r["w0"] and g["sch_ptm"][i] == s["ptm"] and g["sch_amp"][i] == s["amp"] and g["sch_toa"][i] == s["toa"], what
            assert np.array_equal(g["soft"][i, :148], s["soft"]), (what, np.abs(g["soft"][i, :148] - s["soft"]).max())
            assert (bool(g["ok"][i]), int(g["bsic"][i]), int(g["rfn"][i])) == (r["ok"], r["bsic"], r["rfn"]), what
            if name == "FIT + MLSE":
                assert q[i] == s["ptm"] and R[i] == s["R"] and R[i] > 0, what
                assert np.array_equal(chan[i], s["chan"]) and int(win[i]) == s["win"] and s["win"] <= 0, what
            at = r["w0"] + float(s["toa"])
            fn = min(case["sch"], key=lambda p: abs(p[1] - at))[0]
            n15[name] += int(r["state"] == 15 and (r["bsic"], r["rfn"]) == (case["bsic"], fn))
    print("sps %d: streams at state 15 with the right FN and BSIC: %s" % (sps, n15))
    assert n15["FIT + MLSE"] == len(rig.streams) and n15["VALLEY + MLSE"] < len(rig.streams) and n15["VALLEY + DEMOD"] < len(rig.streams)


def test_negative_streams_under_fit(rig):
    pkg, sps = rig.pkg, rig.sps
    neg = am.negative_streams(rig.o, rig.tx, sps)
    acq = pkg.L1Acq(rig.ctx, 1, max(len(x) for _, x in neg))
    acq.set_sch_detector(pkg.SCHDET_FIT)
    acq.set_sch_leg(pkg.SCHLEG_MLSE)
    det = ff.fit_detector(sps, True)
    for name, x in neg:
        d_x = dev(np.ascontiguousarray(x).view(np.float32))
        acq.search(d_x, len(x), len(x), 1, 0.5, FIT_THRESH)
        g = acq.collect()
        q, R = acq.sch_fit()
        r = am.search_model(det, rig.tx, x, 0.5, FIT_THRESH, k=int(g["fcch_k"][0]), omega=g["omega"][0])
        assert int(g["state"][0]) == r["state"] and not g["state"][0] & 4, (name, int(g["state"][0]), r["state"])
        assert g["sch_ptm"][0] == q[0] == (r["sch"]["ptm"] if r["sch"] else 0), name
    acq.destroy()


def test_refusals(rig):
    import ctypes as C
    pkg, L = rig.pkg, rig.ctx.L
    acq = pkg.L1Acq(rig.ctx, 2, 1000)
    for det in (2, -1, 255):
        assert L.trxsig_l1acq_set_sch_detector(acq.h, det) == EINVAL
        with pytest.raises(pkg.TrxSigError):
            acq.set_sch_detector(det)
    a, b = C.c_void_p(), C.c_void_p()
    assert L.trxsig_l1acq_sch_fit(acq.h, None, C.byref(b)) == EINVAL and L.trxsig_l1acq_sch_fit(acq.h, C.byref(a), None) == EINVAL
    assert L.trxsig_l1acq_sch_fit(acq.h, C.byref(a), C.byref(b)) == 0 and a.value and b.value
    for det in (pkg.SCHDET_FIT, pkg.SCHDET_VALLEY):
        for leg in (pkg.SCHLEG_MLSE, pkg.SCHLEG_DEMOD):
            acq.set_sch_detector(det); acq.set_sch_leg(leg)
    rig.ctx.synchronize()
    acq.destroy()
