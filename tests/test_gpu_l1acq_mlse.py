"""Acquisition's SCH leg on the GPU (trxsig_l1acq_set_sch_leg, trxsig_l1acq_sch_channel; include/trxsig_l1acq.h), at sps 1 and 4.

  DEMOD leg   after the setter has been called and set back, trxsig_l1acq_search and trxsig_l1acq_detect_sch_batch give a fresh
              object's outputs byte for byte; trxsig_l1acq_sch_channel hands out zeros and 2
  MLSE leg    flags, amp, toa and ptm are the DEMOD leg's byte for byte; soft and hard equal tests/mlse_sch_model.py on the
              model's shifted windows (tests/mlse_sch_family.py's MlseSchDetector); the taps and window words equal the model's
  a search    four streams of tests/l1_acq_model.py's N_FRAMES through a fixed tap set with three symbols of spread: d_state, d_rfn
              and d_bsic on each leg equal what l1_acq_model.search_model predicts for that leg (fed with the window and the shift
              the library reported, as tests/test_gpu_l1acq.py does); the tap set is chosen so that the model predicts state 15 on
              every stream for the MLSE leg and fewer for the DEMOD leg -- at sch_thresh = 2.5, for no tap set does so at the default
              (tests/mlse_sch_family.py says why)."""
import numpy as np
import pytest

import l1_acq_model as am
import mlse_sch_family as family
from mlse_run import dev, pkg  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu
EINVAL = -1
KEYS = ("state", "fcch_k", "fcch_metric", "fcch_c", "fcch_e", "arg", "omega", "sch_w0", "sch_ptm", "sch_amp", "sch_toa", "soft", "ok", "bsic", "rfn")


class Rig:
    def __init__(self, pkg, sps):
        self.pkg, self.sps = pkg, sps
        self.ctx = pkg.TrxSig(sps, 0)
        self.ctx.use_torch_stream()
        self.det = family.detector(sps)
        self.mdet = family.MlseSchDetector(self.det.o)
        self.tx = family._tx()
        self.streams = family.search_streams(sps)
        N = len(self.streams[0][0])
        self.N, self.stride = N, N + 3
        buf = np.zeros((len(self.streams), self.stride), np.complex64)
        for i, (x, _) in enumerate(self.streams):
            buf[i, :N] = x
        self.flat = buf.ravel()
        self.d = dev(self.flat.view(np.float32))

    def search(self, acq):
        acq.search(self.d, self.stride, self.N, len(self.streams), 0.5, family.SEARCH_SCH_THRESH)
        return acq.collect()

    def windows(self):
        """(off, len, omega) into the flat buffer: per stream the window a search would cut round its first whole SCH burst, one cut
        two symbols short of 148 behind the burst's start and one of 100 symbols from the middle of the burst on (neither can be
        detected, on either leg)."""
        sps = self.sps
        off, ln, om = [], [], []
        for i, (x, case) in enumerate(self.streams):
            at = next(int(p) for _, p in case["sch"] if p >= 12 * sps and p + 180 * sps <= self.N)
            o = np.float32(-2 * np.pi * case["f"] / sps)
            for a, n in ((at - 12 * sps, 172 * sps), (at - 12 * sps, 158 * sps), (at + 74 * sps, 100 * sps)):
                off.append(i * self.stride + a); ln.append(n); om.append(o)
        return np.array(off, np.int32), np.array(ln, np.int32), np.array(om, np.float32)

    def detect(self, acq):
        import torch
        off, ln, om = self.windows()
        B = len(off)
        flags, amp, toa, ptm = (torch.full((B,), 77, dtype=torch.uint8).cuda(), torch.ones(B, 2).cuda(), torch.ones(B).cuda(), torch.ones(B).cuda())
        soft, hard = torch.full((B, 150), -1.0).cuda(), torch.full((B, 150), 255, dtype=torch.uint8).cuda()
        acq.detect_sch(self.d, dev(off), dev(ln), flags, amp, toa, soft, omega=dev(om), ptm=ptm, hard=hard, detect_thresh=family.SEARCH_SCH_THRESH)
        self.ctx.synchronize()
        return dict(flags=flags.cpu().numpy(), amp=amp.cpu().numpy().view(np.complex64).ravel(), toa=toa.cpu().numpy(), ptm=ptm.cpu().numpy(),
                    soft=soft.cpu().numpy(), hard=hard.cpu().numpy())


@pytest.fixture(scope="module", params=[1, 4])
def rig(request, pkg):
    return Rig(pkg, request.param)


@pytest.fixture(scope="module")
def legs(rig):
    """One search and one detect_sch_batch per leg, shared: (fresh object on DEMOD, one object switched to MLSE and back again)."""
    pkg = rig.pkg
    S = len(rig.streams)
    fresh = pkg.L1Acq(rig.ctx, S, rig.N)
    out = dict(fresh_search=rig.search(fresh), fresh_detect=rig.detect(fresh), fresh_channel=fresh.sch_channel())
    fresh.destroy()
    acq = pkg.L1Acq(rig.ctx, S, rig.N)
    acq.set_sch_leg(pkg.SCHLEG_MLSE)
    out["mlse_search"] = rig.search(acq)
    out["mlse_channel"] = acq.sch_channel()
    out["mlse_detect"] = rig.detect(acq)
    out["mlse_channel_after_detect"] = acq.sch_channel()
    acq.set_sch_leg(pkg.SCHLEG_DEMOD)
    out["back_search"] = rig.search(acq)
    out["back_detect"] = rig.detect(acq)
    out["back_channel"] = acq.sch_channel()
    acq.destroy()
    return out


def test_demod_leg_is_unchanged_by_a_byte(rig, legs):
    """Set to MLSE, used, and set back: every output of search and detect_sch_batch equals a fresh object's byte for byte, and the
    channel accessor hands out zeros and 2 on this leg."""
    for k in KEYS:
        assert legs["back_search"][k].tobytes() == legs["fresh_search"][k].tobytes(), "search: " + k
    for k in legs["fresh_detect"]:
        assert legs["back_detect"][k].tobytes() == legs["fresh_detect"][k].tobytes(), "detect_sch_batch: " + k
    assert (legs["fresh_search"]["state"] & 4).all()           # (the streams do reach the leg)
    for name in ("fresh_channel", "back_channel"):
        chan, win = legs[name]
        assert chan.shape == (len(rig.streams), 5) and not chan.any() and (win == 2).all(), name


def test_mlse_leg_detect_sch_batch(rig, legs):
    """Flags, amp, toa and ptm do not depend on the leg; soft and hard are the model's on the model's shifted windows; nothing is
    written past 148 values; the channel accessor still shows the last SEARCH."""
    d, m = legs["fresh_detect"], legs["mlse_detect"]
    for k in ("flags", "amp", "toa", "ptm"):
        assert m[k].tobytes() == d[k].tobytes(), k
    off, ln, om = rig.windows()
    seen = set()
    for b in range(len(off)):
        want = rig.mdet.detect(rig.flat[off[b]:off[b] + ln[b]], om[b], family.SEARCH_SCH_THRESH)
        what = "sps %d window %d" % (rig.sps, b)
        assert m["flags"][b] == want["flags"] and m["amp"][b] == want["amp"] and m["toa"][b] == want["toa"] and m["ptm"][b] == want["ptm"], what
        assert np.array_equal(m["soft"][b, :148], want["soft"]), (what, np.abs(m["soft"][b, :148] - want["soft"]).max())
        assert np.array_equal(m["hard"][b, :148], (want["soft"] > 0.5).astype(np.uint8)), what
        seen.add((int(want["flags"]), int(want["win"])))
    assert (m["soft"][:, 148:] == -1).all() and (m["hard"][:, 148:] == 255).all()
    assert (m["flags"][0::3] == 2).all() and not m["flags"][1::3].any() and not m["flags"][2::3].any()
    assert all(w <= 0 for f, w in seen if f == 2) and (0, 2) in seen
    assert not np.array_equal(m["soft"][0::3, :148], d["soft"][0::3, :148])      # (the legs do differ on these windows)
    for a, b in zip(legs["mlse_channel"], legs["mlse_channel_after_detect"]):
        assert a.tobytes() == b.tobytes()


def test_search_on_both_legs(rig, legs):
    """Per stream and leg: state, w0, ptm, amp, toa, soft, ok, bsic and rfn equal l1_acq_model.search_model with that leg's detector
    (fed with the library's window and shift); stage 1, flags, amp, toa, ptm and state bits 1, 2 and 4 are the same bytes on both
    legs; trxsig_l1acq_sch_channel equals the model's taps and window words.  The model predicts state 15 with the right FN and
    BSIC on every stream for the MLSE leg and on fewer for the DEMOD leg."""
    gd, gm = legs["fresh_search"], legs["mlse_search"]
    for k in ("fcch_k", "fcch_metric", "fcch_c", "fcch_e", "arg", "omega", "sch_w0", "sch_ptm", "sch_amp", "sch_toa"):
        assert gm[k].tobytes() == gd[k].tobytes(), k
    assert np.array_equal(gm["state"] & 7, gd["state"] & 7)
    chan, win = legs["mlse_channel"]
    n15 = {}
    for leg, g, det in (("DEMOD", gd, rig.det), ("MLSE", gm, rig.mdet)):
        n15[leg] = 0
        for i, (x, case) in enumerate(rig.streams):
            what = "sps %d %s stream %d" % (rig.sps, leg, i)
            r = am.search_model(det, rig.tx, x, 0.5, family.SEARCH_SCH_THRESH, k=int(g["fcch_k"][i]), omega=g["omega"][i])
            assert int(g["state"][i]) == r["state"], (what, int(g["state"][i]), r["state"])
            assert r["state"] & 4, what
            s = r["sch"]
            assert int(g["sch_w0"][i]) == r["w0"] and g["sch_ptm"][i] == s["ptm"] and g["sch_amp"][i] == s["amp"] and g["sch_toa"][i] == s["toa"], what
            assert np.array_equal(g["soft"][i, :148], s["soft"]), (what, np.abs(g["soft"][i, :148] - s["soft"]).max())
            assert (bool(g["ok"][i]), int(g["bsic"][i]), int(g["rfn"][i])) == (r["ok"], r["bsic"], r["rfn"]), what
            if leg == "MLSE":
                assert np.array_equal(chan[i], s["chan"]) and int(win[i]) == s["win"] and s["win"] <= 0, what
            at = r["w0"] + float(s["toa"])
            fn = min(case["sch"], key=lambda p: abs(p[1] - at))[0]
            n15[leg] += int(r["state"] == 15 and (r["bsic"], r["rfn"]) == (case["bsic"], fn))
    print("sps %d: streams at state 15 with the right FN and BSIC: DEMOD leg %d, MLSE leg %d of %d" % (rig.sps, n15["DEMOD"], n15["MLSE"], len(rig.streams)))
    assert n15["MLSE"] == len(rig.streams) and n15["DEMOD"] < len(rig.streams)


def test_refusals(rig):
    import ctypes as C
    pkg, L = rig.pkg, rig.ctx.L
    acq = pkg.L1Acq(rig.ctx, 2, 1000)
    for leg in (2, -1, 255):
        assert L.trxsig_l1acq_set_sch_leg(acq.h, leg) == EINVAL
        with pytest.raises(pkg.TrxSigError):
            acq.set_sch_leg(leg)
    a, b = C.c_void_p(), C.c_void_p()
    assert L.trxsig_l1acq_sch_channel(acq.h, None, C.byref(b)) == EINVAL and L.trxsig_l1acq_sch_channel(acq.h, C.byref(a), None) == EINVAL
    assert L.trxsig_l1acq_sch_channel(acq.h, C.byref(a), C.byref(b)) == 0 and a.value and b.value
    acq.set_sch_leg(pkg.SCHLEG_MLSE); acq.set_sch_leg(pkg.SCHLEG_DEMOD)
    rig.ctx.synchronize()
    acq.destroy()
