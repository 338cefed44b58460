"""GPU parity of the fit detector's statistic (trxsig_sch_fit_batch, csrc/trxsig_sch_fit.hip) against its float32 model
(tests/sch_fit_model.py): the nine taps, the window word, E, R and q are IEEE-equal -- at sps 1, 2 and 4, on batches of 1, 3, 9 and
37 bursts of tests/mlse_sch_family.mixed_batch and on its hostile bursts that must fall back or be skipped (NaN, infinity, 2^30,
zeros, short bursts, TOA +-4096, disabled bursts).  The kernel takes two bursts a wave, one after the other, and eight a workgroup:
B = 1 leaves a wave's second turn empty, B = 3 ends inside the second wave, B = 9 puts a workgroup one burst over, B = 37 is four
workgroups and a ragged fifth.  Every output array carries canaries behind its last entry."""
import numpy as np
import pytest

import mlse_sch_family as family
import sch_fit_model as model
import sch_fit_ref as ref
from mlse_run import ctx, pkg, run_fit  # noqa: F401  (the fixtures)
from util import GpuBatch, assert_veq

pytestmark = pytest.mark.gpu
B_ALL = 37


def check(got, want, sel=None, what=""):
    sel = slice(None) if sel is None else sel
    assert_veq(got["win"], want["win"][sel], what + " window word")
    for k in ("chan9", "E", "R", "q"):
        assert_veq(got[k], want[k][sel], what + " " + k)


@pytest.fixture(scope="module")
def wanted():
    out = {}
    for sps in (1, 2, 4):
        f = family.mixed_batch(sps, B_ALL, 6100 + sps)
        out[sps] = (f, model.fit_batch(sps, f["x"], f["off"], f["length"], f["amp"], f["toa"]))
    return out


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_model_parity(ctx, wanted, sps):
    """37 bursts: every output equals the model and lies within the float64 bound; a repeat is byte-equal; B = 1, 3 and 9, the
    batch's tail and a middle stretch give the batch's own values; each output alone (the others NULL) gives its own values."""
    f, want = wanted[sps]
    on = want["win"] <= 0
    assert on.sum() >= 33 and len(set(want["win"].tolist())) >= 3 and np.isfinite(want["q"]).all() and (want["q"][on] > 1.4).all()
    got = run_fit(ctx[sps], f)
    check(got, want, what="sps %d" % sps)
    g = ref.grade(got["R"][on], got["q"][on], want["y"][on], want["w"][on], want["h"][on])
    print("sps %d: worst error / bound on %d bursts: R %.3f, q %.3f" % (sps, on.sum(), g["ratio_R"].max(), g["ratio_q"].max()))
    assert g["ok_R"].all() and g["ok_q"].all()
    again = run_fit(ctx[sps], f)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), "repeat differs: " + k
    for sel in (np.arange(1), np.arange(3), np.arange(9), np.arange(32, 37), np.arange(5, 22)):
        part = run_fit(ctx[sps], f, sel=sel)
        for k in got:
            assert part[k].tobytes() == got[k][sel].tobytes(), "B = %d differs from the batch: %s" % (len(sel), k)
    for k in got:
        assert run_fit(ctx[sps], f, sel=np.arange(9), only=k)[k].tobytes() == got[k][:9].tobytes(), "alone: " + k


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_hostile_bursts(ctx, sps):
    """What trxsig_mlse_sch_batch falls back on or skips gets q = 0, E = 0, R = 0, zero taps and the window word 1 or 2 -- all-zero
    samples among them: E == 0 and R == 0 there, and q is the stated 0, not the NaN of 0 / 0; the neighbours are fitted."""
    f = family.hostile_batch(sps)
    want = model.fit_batch(sps, f["x"], f["off"], f["length"], f["amp"], f["toa"], enable=f["enable"])
    assert np.array_equal(want["win"], f["want"]["win"])       # the equaliser's own words
    out_ = want["win"] > 0
    assert out_.sum() >= 12 and (~out_).sum() >= 5 and (want["q"][~out_] > 1.4).all()
    for k in ("chan9", "E", "R", "q"):
        assert not want[k][out_].any(), k
    assert want["win"][f["kind"].index("zeros")] == 1
    got = run_fit(ctx[sps], f, enable=f["enable"])
    check(got, want, what="hostile sps %d" % sps)
    assert not np.isnan(got["q"]).any() and not np.isnan(got["R"]).any()


def test_enable_and_refusals(pkg, ctx, wanted):
    """d_enable skips; NULL inputs are refused (TRXSIG_EINVAL); an empty batch is a no-op."""
    import torch
    f, _ = wanted[4]
    enable = (np.arange(B_ALL) % 3 != 1).astype(np.uint8)
    want = model.fit_batch(4, f["x"], f["off"], f["length"], f["amp"], f["toa"], enable=enable)
    assert (want["win"] == 2).sum() == int((enable == 0).sum())
    check(run_fit(ctx[4], f, enable=enable), want, what="d_enable")
    t = ctx[4]
    gb = GpuBatch(f["x"], f["off"][:4], f["length"][:4], stride=148)
    d_amp = torch.from_numpy(f["amp"][:4].view(np.float32).copy()).cuda(); d_toa = torch.from_numpy(f["toa"][:4].copy()).cuda()
    q = torch.full((4,), -7.0, device="cuda:0")
    for a in ((None, gb.off, gb.len, d_amp, d_toa), (gb.x, gb.off, gb.len, None, d_toa), (gb.x, gb.off, gb.len, d_amp, None)):
        with pytest.raises(pkg.TrxSigError):
            t.sch_fit(*a, q=q)
    t.sch_fit(gb.x, gb.off[:0], gb.len[:0], d_amp, d_toa, q=q)
    t.sch_fit(gb.x, gb.off, gb.len, d_amp, d_toa)              # every output NULL: nothing to write, no fault
    t.synchronize()
    assert np.all(q.cpu().numpy() == -7.0)
