"""GPU parity of the access-burst sequence equaliser (trxsig_mlse_access_batch / trxsig_mlse_rach_batch,
csrc/trxsig_mlse_access.hip) against its float32 model (tests/mlse_access_model.py): soft bits, hard bits, taps and the window word
are IEEE-equal -- at sps 1, 2 and 4, on batches of 1, 3, 5 (a partial wave of four bursts) and 37 bursts (two workgroups of 16 and
a partial one), clean, noisy and multipath bursts, 156- and 157-symbol lengths, odd sample offsets (the non-wide staging path),
delays up to 60 symbols, TOAs on and off the 1/512 grid, and on the hostile bursts that must fall back or be skipped."""
import numpy as np
import pytest

import mlse_access_family as family
import mlse_access_model as model
import oraclebind
from mlse_run import check, ctx, pkg, run_access  # noqa: F401  (the fixtures)
from util import GpuBatch, assert_veq, assert_veq_nan

pytestmark = pytest.mark.gpu
B_ALL = 37


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_model_parity(ctx, sps):
    """37 bursts: every output equals the model; a repeat is bit-equal; B = 1, 3 and 5 and the batch's tail give the batch's own
    values (the layout does not depend on where in a wave or a workgroup a burst lies)."""
    f = family.mixed_batch(sps, B_ALL, 5100 + sps)
    want = f["want"]
    assert (want["win"] <= 0).sum() >= 33 and len(set(want["win"].tolist())) >= 3      # the family does get equalised, in several windows
    ber = ((want["soft"][:, family.PAYLOAD] > 0.5) != f["bits"][:, family.PAYLOAD]).mean()
    assert ber < 0.05, ber                                     # ... and to the bits that were sent
    got = run_access(ctx[sps], f)
    check(got, want, what="sps %d" % sps)
    again = run_access(ctx[sps], f)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), "repeat differs: " + k
    for sel in (np.arange(1), np.arange(3), np.arange(5), np.arange(32, 37), np.arange(6, 23)):
        part = run_access(ctx[sps], f, sel=sel)
        for k in got:
            assert part[k].tobytes() == got[k][sel].tobytes(), "B = %d differs from the batch: %s" % (len(sel), k)


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_hostile_bursts(ctx, sps):
    """All-zero samples, a NaN sample, an infinite one, a component of 2^31, 147 symbols and a tiny amplitude fall back to the
    demodulator's soft bits (window word 1, taps zero); d_enable == 0 is skipped (window word 2, zeros); their neighbours are
    equalised.  Where NaNs are expected the rule is "both NaN, or IEEE ==" (util.veq_nan)."""
    f = family.hostile_batch(sps)
    want = f["want"]
    kind = f["kind"]
    for b, k in enumerate(kind):
        assert (want["win"][b] == 2) if k == "disabled" else ((want["win"][b] <= 0) if k == "plain" else (want["win"][b] == 1)), (k, want["win"][b])
    assert np.isnan(want["soft"][kind.index("nan")]).any()
    got = run_access(ctx[sps], f, enable=f["enable"])
    check(got, want, what="hostile sps %d" % sps)
    # the fallback IS the demodulator: the same bursts through trxsig_demodulate_batch
    import torch
    gb = GpuBatch(f["x"], f["off"], f["length"], nsoft=148, stride=148)
    d_amp = torch.from_numpy(f["amp"].view(np.float32).copy()).cuda(); d_toa = torch.from_numpy(f["toa"]).cuda()
    ctx[sps].demodulate(gb.x, gb.off, gb.len, d_amp, d_toa, gb.soft, nsoft=148)
    dem = gb.results()["soft"]
    for b, k in enumerate(kind):
        n = min(148, int(f["length"][b]) // sps)
        if want["win"][b] == 1:
            assert_veq_nan(got["soft"][b, :n], dem[b, :n], "fallback burst %d (%s) against the demodulator" % (b, k))
        elif want["win"][b] <= 0:                               # an equalised burst keeps the demodulator's bits off the trellis
            assert_veq(got["soft"][b, :49], dem[b, :49], "burst %d, the known head" % b)
            assert_veq(got["soft"][b, 88:148], dem[b, 88:148], "burst %d, behind the tail" % b)
            assert np.all(got["soft"][b, 85:88] == 0.0), "burst %d: the tail bits are not exactly 0" % b


def test_nsoft_and_null_outputs(ctx):
    """nsoft in {85, 88, 148} (and 0, 49, 50) with stride 160 writes only that many; d_chan, d_win and d_hard may be NULL;
    d_enable skips."""
    f = family.mixed_batch(4, B_ALL, 5104)
    sel = np.arange(9)
    for nsoft in (85, 88, 148, 0, 49, 50):
        got = run_access(ctx[4], f, sel=sel, nsoft=nsoft, stride=160)
        check(got, f["want"], sel=sel, nsoft=nsoft, what="nsoft %d" % nsoft)
    got = run_access(ctx[4], f, sel=sel, with_aux=False)
    assert_veq(got["soft"][:, :148], f["want"]["soft"][sel], "soft bits without d_chan / d_win")
    got = run_access(ctx[4], f, sel=sel, with_hard=False)
    assert_veq(got["soft"][:, :148], f["want"]["soft"][sel], "soft bits without d_hard")
    assert np.all(got["hard"] == 255), "d_hard == NULL, and hard bits were written somewhere"
    enable = (np.arange(B_ALL) % 3 != 1).astype(np.uint8)
    want = model.access_batch(4, f["x"], f["off"], f["length"], f["amp"], f["toa"], enable=enable)
    assert (want["win"] == 2).sum() == int((enable == 0).sum())
    check(run_access(ctx[4], f, enable=enable), want, what="d_enable")


@pytest.mark.parametrize("sps", [1, 4])
def test_mlse_rach_batch(pkg, ctx, sps):
    """trxsig_mlse_rach_batch: flags, amplitude, TOA and avgPwr are trxsig_detect_demod_rach_batch's in both soft modes; the soft
    bits are trxsig_mlse_access_batch's (and the model's) on the detected bursts with those amplitudes and TOAs, zeros (window word
    2) on the others."""
    import torch
    f = family.mixed_batch(sps, B_ALL, 5100 + sps)
    t = ctx[sps]
    ref = GpuBatch(f["x"], f["off"], f["length"])
    t.detect_demod_rach(ref.x, ref.off, ref.len, ref.flags, ref.amp, ref.toa, ref.soft, avgpwr=ref.pwr, energy_thresh=-1.0)
    r0 = ref.results()
    det = (r0["flags"] & pkg.F_DETECT) != 0
    assert det.sum() >= 15 and (~det).sum() >= 1, det.sum()
    fd = dict(f, amp=r0["amp"], toa=r0["toa"])
    direct = run_access(t, fd, enable=det.astype(np.uint8))
    want = model.access_batch(sps, f["x"], f["off"], f["length"], r0["amp"], r0["toa"], enable=det.astype(np.uint8), oracle=oraclebind.Oracle(sps))
    assert np.all(want["soft"][~det] == 0) and np.all(want["win"][~det] == 2)
    try:
        for mode in (pkg.SOFT_EXACT, pkg.SOFT_TOLERANCE):
            t.set_soft_mode(mode)
            gb = GpuBatch(f["x"], f["off"], f["length"], stride=160)
            chan = torch.zeros((B_ALL, 5, 2), dtype=torch.float32, device="cuda:0"); win = torch.zeros(B_ALL, dtype=torch.int32, device="cuda:0")
            t.mlse_rach(gb.x, gb.off, gb.len, gb.flags, gb.amp, gb.toa, gb.soft, avgpwr=gb.pwr, chan=chan, win=win, hard=gb.hard,
                        energy_thresh=-1.0, soft_stride=160)
            r = gb.results()
            for k in ("flags", "amp", "toa", "pwr"):
                assert r[k].tobytes() == r0[k].tobytes(), "mode %d: %s differs from trxsig_detect_demod_rach_batch" % (mode, k)
            got = dict(soft=r["soft"], hard=r["hard"], chan=chan.cpu().numpy().reshape(B_ALL, 10).view(np.complex64), win=win.cpu().numpy())
            check(got, want, what="mlse_rach mode %d" % mode)
            for k in got:
                assert got[k].tobytes() == direct[k].tobytes(), "mode %d: %s differs from trxsig_mlse_access_batch" % (mode, k)
    finally:
        t.set_soft_mode(pkg.SOFT_EXACT)


def test_refusals(pkg, ctx):
    """nsoft > 148, a stride below nsoft and NULL arrays are refused (TRXSIG_EINVAL); an empty batch is a no-op."""
    import torch
    f = family.mixed_batch(4, B_ALL, 5104)
    t = ctx[4]
    gb = GpuBatch(f["x"], f["off"][:4], f["length"][:4], stride=160)
    d_amp = torch.from_numpy(f["amp"][:4].view(np.float32).copy()).cuda(); d_toa = torch.from_numpy(f["toa"][:4].copy()).cuda()
    for kw in (dict(nsoft=149), dict(nsoft=-1), dict(nsoft=148, soft_stride=147), dict(amp=None), dict(toa=None), dict(soft=None, soft_stride=160)):
        a = dict(amp=d_amp, toa=d_toa, soft=gb.soft, nsoft=148, soft_stride=160); a.update(kw)
        with pytest.raises(pkg.TrxSigError):
            t.mlse_access(gb.x, gb.off, gb.len, a["amp"], a["toa"], a["soft"], nsoft=a["nsoft"], soft_stride=a["soft_stride"])
    with pytest.raises(pkg.TrxSigError):
        t.mlse_rach(gb.x, gb.off, gb.len, gb.flags, gb.amp, gb.toa, gb.soft, nsoft=149, soft_stride=160)
    t.mlse_access(gb.x, gb.off[:0], gb.len[:0], d_amp, d_toa, gb.soft, soft_stride=160)
    torch.cuda.synchronize()
    assert np.all(gb.soft.cpu().numpy() == -1.0)
