"""GPU parity of the sequence equaliser (trxsig_mlse_batch / trxsig_mlse_normal_batch, csrc/trxsig_mlse.hip) against its float32
model (tests/mlse_model.py): soft bits, hard bits, taps and the window word are IEEE-equal -- on clean, noisy and multipath
bursts at sps 1, 2 and 4, every training sequence, 156- and 157-symbol bursts, odd sample offsets (the non-wide staging path),
TOAs across +-3 symbols on and off the 1/512 grid, and on the hostile bursts that must fall back or be skipped."""
import numpy as np
import pytest

import mlse_family
import mlse_model
import oraclebind
from mlse_run import check, ctx, pkg, run_mlse  # noqa: F401  (the fixtures)
from util import GpuBatch, assert_veq, assert_veq_nan

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_model_parity_67(ctx, sps):
    """67 bursts (33 full waves and a half one at two bursts a wave): every output equals the model; a repeat is bit-equal; 64 + 3
    bursts give what 67 give; B = 1 and B = 5 give the batch's first bursts."""
    f = mlse_family.mixed_batch(sps, 2, 67, 4100 + sps)
    want = f["want"]
    assert (want["win"] <= 0).sum() >= 60 and len(set(want["win"].tolist())) >= 3      # the family does get equalised, in several windows
    got = run_mlse(ctx[sps], f)
    check(got, want, what="sps %d" % sps)
    again = run_mlse(ctx[sps], f)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), "repeat differs: " + k
    for sel in (np.arange(64), np.arange(64, 67), np.arange(1), np.arange(5)):
        part = run_mlse(ctx[sps], f, sel=sel)
        for k in got:
            assert part[k].tobytes() == got[k][sel].tobytes(), "B = %d differs from the batch: %s" % (len(sel), k)


@pytest.mark.parametrize("tsc", range(8))
def test_every_training_sequence(ctx, tsc):
    f = mlse_family.mixed_batch(4, tsc, 5, 4200 + tsc)
    check(run_mlse(ctx[4], f), f["want"], what="tsc %d" % tsc)
    f1 = mlse_family.mixed_batch(1, tsc, 5, 4300 + tsc)
    check(run_mlse(ctx[1], f1), f1["want"], what="tsc %d sps 1" % tsc)


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_hostile_bursts(ctx, sps):
    """All-zero samples, a NaN sample, an infinite one, a component of 2^31, 147 symbols and a tiny amplitude fall back to the
    demodulator's soft bits (window word 1, taps zero); d_enable == 0 is skipped (window word 2, zeros); their neighbours are
    equalised.  Where NaNs are expected the rule is "both NaN, or IEEE ==" (util.veq_nan)."""
    f = mlse_family.hostile_batch(sps)
    want = f["want"]
    kind = f["kind"]
    for b, k in enumerate(kind):
        assert (want["win"][b] == 2) if k == "disabled" else ((want["win"][b] <= 0) if k == "plain" else (want["win"][b] == 1)), (k, want["win"][b])
    assert np.isnan(want["soft"][kind.index("nan")]).any()
    got = run_mlse(ctx[sps], f, enable=f["enable"])
    check(got, want, what="hostile sps %d" % sps)
    # the fallback IS the demodulator: the same bursts through trxsig_demodulate_batch
    import torch
    gb = GpuBatch(f["x"], f["off"], f["length"], nsoft=148, stride=148)
    d_amp = torch.from_numpy(f["amp"].view(np.float32).copy()).cuda(); d_toa = torch.from_numpy(f["toa"]).cuda()
    ctx[sps].demodulate(gb.x, gb.off, gb.len, d_amp, d_toa, gb.soft, nsoft=148)
    dem = gb.results()["soft"]
    for b, k in enumerate(kind):
        if want["win"][b] == 1:
            n = min(148, int(f["length"][b]) // sps)
            assert_veq_nan(got["soft"][b, :n], dem[b, :n], "fallback burst %d (%s) against the demodulator" % (b, k))


def test_nsoft_and_null_outputs(ctx):
    """nsoft < 148 writes only that many; d_chan, d_win and d_hard may be NULL."""
    f = mlse_family.mixed_batch(4, 2, 67, 4104)
    sel = np.arange(9)
    for nsoft in (0, 61, 100):
        got = run_mlse(ctx[4], f, sel=sel, nsoft=nsoft, stride=148)
        check(got, f["want"], sel=sel, nsoft=nsoft, what="nsoft %d" % nsoft)
    got = run_mlse(ctx[4], f, sel=sel, with_aux=False)
    assert_veq(got["soft"][:, :148], f["want"]["soft"][sel], "soft bits without d_chan / d_win")


@pytest.mark.parametrize("sps", [1, 4])
def test_mlse_normal_batch(pkg, ctx, sps):
    """trxsig_mlse_normal_batch: flags, amplitude, TOA and avgPwr are trxsig_detect_demod_normal_batch's in both soft modes; the soft
    bits are the model's on the detected bursts with those amplitudes and TOAs, zeros (window word 2) on the others."""
    import torch
    f = mlse_family.mixed_batch(sps, 2, 67, 4100 + sps)
    t = ctx[sps]
    ref = GpuBatch(f["x"], f["off"], f["length"])
    t.detect_demod_normal(ref.x, ref.off, ref.len, f["tsc"], ref.flags, ref.amp, ref.toa, ref.soft, avgpwr=ref.pwr, energy_thresh=-1.0)
    r0 = ref.results()
    det = (r0["flags"] & pkg.F_DETECT) != 0
    assert det.sum() >= 40 and (~det).sum() >= 0
    o = oraclebind.Oracle(sps)
    want = mlse_model.mlse_batch(sps, f["x"], f["off"], f["length"], f["tsc"], r0["amp"], r0["toa"], enable=det.astype(np.uint8), oracle=o)
    try:
        for mode in (pkg.SOFT_EXACT, pkg.SOFT_TOLERANCE):
            t.set_soft_mode(mode)
            gb = GpuBatch(f["x"], f["off"], f["length"], stride=160)
            chan = torch.zeros((67, 5, 2), dtype=torch.float32, device="cuda:0"); win = torch.zeros(67, dtype=torch.int32, device="cuda:0")
            t.mlse_normal(gb.x, gb.off, gb.len, f["tsc"], gb.flags, gb.amp, gb.toa, gb.soft, avgpwr=gb.pwr, chan=chan, win=win, hard=gb.hard,
                          energy_thresh=-1.0, soft_stride=160)
            r = gb.results()
            for k in ("flags", "amp", "toa", "pwr"):
                assert r[k].tobytes() == r0[k].tobytes(), "mode %d: %s differs from trxsig_detect_demod_normal_batch" % (mode, k)
            got = dict(soft=r["soft"], hard=r["hard"], chan=chan.cpu().numpy().reshape(67, 10).view(np.complex64), win=win.cpu().numpy())
            check(got, want, what="mlse_normal mode %d" % mode)
    finally:
        t.set_soft_mode(pkg.SOFT_EXACT)


def test_refusals(pkg, ctx):
    """nsoft > 148, tsc outside 0..7, a stride below nsoft and NULL arrays are refused (TRXSIG_EINVAL); an empty batch is a no-op."""
    import torch
    f = mlse_family.mixed_batch(4, 2, 67, 4104)
    t = ctx[4]
    gb = GpuBatch(f["x"], f["off"][:4], f["length"][:4], stride=160)
    d_amp = torch.from_numpy(f["amp"][:4].view(np.float32).copy()).cuda(); d_toa = torch.from_numpy(f["toa"][:4].copy()).cuda()
    for kw in (dict(nsoft=149), dict(nsoft=-1), dict(tsc=8), dict(tsc=-1), dict(nsoft=148, soft_stride=147), dict(amp=None), dict(toa=None),
               dict(soft=None, soft_stride=160)):
        a = dict(tsc=2, amp=d_amp, toa=d_toa, soft=gb.soft, nsoft=148, soft_stride=160); a.update(kw)
        with pytest.raises(pkg.TrxSigError):
            t.mlse(gb.x, gb.off, gb.len, a["tsc"], a["amp"], a["toa"], a["soft"], nsoft=a["nsoft"], soft_stride=a["soft_stride"])
    with pytest.raises(pkg.TrxSigError):
        t.mlse_normal(gb.x, gb.off, gb.len, 2, gb.flags, gb.amp, gb.toa, gb.soft, nsoft=149, soft_stride=160)
    t.mlse(gb.x, gb.off[:0], gb.len[:0], 2, d_amp, d_toa, gb.soft, soft_stride=160)
    torch.cuda.synchronize()
    assert np.all(gb.soft.cpu().numpy() == -1.0)
