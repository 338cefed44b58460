"""GPU parity of the two-antenna sequence equaliser (trxsig_mlse_div_batch / trxsig_mlse_div_normal_batch,
csrc/trxsig_mlse_div.hip) against its float32 model (tests/mlse_div_model.py): soft bits, hard bits, both tap sets and the window
word are IEEE-equal at sps 1, 2 and 4 -- batches of 1, 2, 3, 9 and 8 + 3 bursts (a wave with one burst, a second workgroup, a
partly filled last one), 156- and 157-symbol bursts, antenna offsets of equal and of different parity, gaps that differ between
the antennas, TOAs off the grid, two training sequences, nsoft 148 and 100; the three identities on the device; the hostile
bursts on either antenna; and the kernel's output graded directly by the float64 reference (tests/mlse_div_ref.py)."""
import numpy as np
import pytest

import mlse_div_family as dfam
import mlse_div_model as dm
import mlse_div_ref as dref
import mlse_family
import mlse_ref
import oraclebind
from mlse_run import check, ctx, dev, pkg, run_div  # noqa: F401  (the fixtures)
from util import GpuBatch, assert_veq

pytestmark = pytest.mark.gpu


def run_one(t, x, off, length, tsc, amp, toa, enable=None):
    """trxsig_mlse_batch on one antenna: dict(soft [B, 148], hard, chan [B, 5], win)."""
    import torch
    B = len(off)
    gb = GpuBatch(x, off, length, nsoft=148, stride=148)
    chan = torch.zeros((B, 5, 2), dtype=torch.float32, device="cuda:0"); win = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    t.mlse(gb.x, gb.off, gb.len, tsc, dev(amp), dev(toa), gb.soft, enable=None if enable is None else dev(enable), chan=chan, win=win,
           hard=gb.hard, nsoft=148, soft_stride=148)
    r = gb.results()
    return dict(soft=r["soft"], hard=r["hard"], chan=chan.cpu().numpy().reshape(B, 10).view(np.complex64), win=win.cpu().numpy())


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_model_parity(ctx, sps):
    """11 bursts of two training sequences: every output equals the model for B = 1, 2, 3, 9 and 8 + 3; nsoft = 100 writes only
    that many; a repeat of one call gives the same bytes; d_chan, d_win and d_hard may be NULL."""
    for tsc in (2, 6):
        f = dfam.mixed_batch(sps, tsc, 11, 6300 + 10 * sps + tsc)
        want = f["want"]
        assert (want["win"] <= 0).sum() >= 9 and (f["length"] == 157 * sps).any() and (f["length"] == 156 * sps).any()
        for B in (1, 2, 3, 9, 11):
            for nsoft in ((148, 100) if B in (3, 11) else (148,)):
                got = run_div(ctx[sps], f, sel=np.arange(B), nsoft=nsoft)
                check(got, want, sel=np.arange(B), nsoft=nsoft, what="sps %d tsc %d B %d nsoft %d" % (sps, tsc, B, nsoft))
        part = run_div(ctx[sps], f, sel=np.arange(8, 11))
        check(part, want, sel=np.arange(8, 11), what="sps %d tsc %d bursts 8..10" % (sps, tsc))
        got = run_div(ctx[sps], f)
        again = run_div(ctx[sps], f)
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), "repeat differs: " + k
        bare = run_div(ctx[sps], f, with_aux=False)
        assert_veq(bare["soft"][:, :148], want["soft"], "soft bits without d_chan / d_win")


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_identities_on_the_device(ctx, sps):
    """Antenna 1 all zeros, and the same samples on both antennas (at another offset, of the other parity): soft bits, hard bits and
    the window are trxsig_mlse_batch's own output on antenna 0; the taps its taps (zeros for the silent antenna).  Antennas swapped
    with d_primary: soft bits and the window identical, the tap sets exchanged."""
    f1 = mlse_family.mixed_batch(sps, 2, 67, 4100 + sps)
    sel = np.arange(19)
    one = run_one(ctx[sps], f1["x"], f1["off"][sel], f1["length"][sel], f1["tsc"], f1["amp"][sel], f1["toa"][sel])
    base = dict(sps=sps, tsc=f1["tsc"], x0=f1["x"], off0=f1["off"][sel], length=f1["length"][sel], amp=f1["amp"][sel], toa=f1["toa"][sel], primary=None)
    for name, x1, off1 in (("zeros", np.zeros_like(f1["x"]), f1["off"][sel]),
                           ("same", np.concatenate([np.zeros(3, np.complex64), f1["x"]]), f1["off"][sel] + 3)):
        got = run_div(ctx[sps], dict(base, x1=x1, off1=off1), stride=148)
        for k in ("soft", "hard", "win"):
            assert got[k].tobytes() == one[k].tobytes(), "%s: %s differs from trxsig_mlse_batch" % (name, k)
        assert got["chan"][:, 0].tobytes() == one["chan"].tobytes()
        assert (not got["chan"][:, 1].any()) if name == "zeros" else (got["chan"][:, 1].tobytes() == one["chan"].tobytes())
    f = dfam.mixed_batch(sps, 2, 11, 6300 + 10 * sps + 2)
    got = run_div(ctx[sps], f)
    swapped = run_div(ctx[sps], dict(f, x0=f["x1"], off0=f["off1"], x1=f["x0"], off1=f["off0"], primary=1 - f["primary"]))
    assert swapped["soft"].tobytes() == got["soft"].tobytes() and swapped["win"].tobytes() == got["win"].tobytes()
    assert swapped["chan"][:, 0].tobytes() == got["chan"][:, 1].tobytes() and swapped["chan"][:, 1].tobytes() == got["chan"][:, 0].tobytes()


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_hostile_bursts_on_either_antenna(ctx, sps):
    """mlse_family.hostile_batch (zeros, a NaN, an infinity, 2^31, 147 symbols, a tiny amplitude, d_enable == 0) as one antenna
    against ordinary bursts on the other, and the reverse, with d_enable and alternating d_primary: everything equals the model;
    the bursts that must fall back do (window word 1), the disabled one is skipped (2), the plain ones are equalised -- and so is
    the one whose hostile antenna is all zeros: a silent antenna beside an ordinary one is the first identity, not a fallback."""
    h = mlse_family.hostile_batch(sps)
    g = mlse_family.mixed_batch(sps, 5, 10, 4400 + sps)
    assert np.all(h["length"] <= g["length"])                 # the antennas share the hostile batch's lengths
    o = oraclebind.Oracle(sps)
    primary = (np.arange(10) % 2).astype(np.uint8)
    for name, a0, a1 in (("hostile first", h, g), ("hostile second", g, h)):
        f = dict(sps=sps, tsc=5, x0=a0["x"], off0=a0["off"], x1=a1["x"], off1=a1["off"], length=h["length"], amp=h["amp"], toa=h["toa"], primary=primary)
        want = dm.mlse_div_batch(sps, f["x0"], f["off0"], f["x1"], f["off1"], f["length"], 5, f["amp"], f["toa"], primary=primary,
                                 enable=h["enable"], oracle=o)
        for b, k in enumerate(h["kind"]):
            assert (want["win"][b] == 2) if k == "disabled" else ((want["win"][b] <= 0) if k in ("plain", "zeros") else (want["win"][b] == 1)), (name, k)
        got = run_div(ctx[sps], f, enable=h["enable"])
        check(got, want, what="%s sps %d" % (name, sps))


@pytest.mark.parametrize("sps", [1, 4])
def test_mlse_div_normal_batch(pkg, ctx, sps):
    """trxsig_mlse_div_normal_batch: flags, amplitude, TOA and avgPwr of each antenna are trxsig_detect_demod_normal_batch's in both
    soft modes; d_sel is select() on them; the soft bits are the model's with the selected antenna's amp and TOA and d_primary =
    d_sel, zeros (window word 2) where neither antenna detected.  Bursts 1, 5 are silent on antenna 0, 2, 6 on antenna 1, 3 on both."""
    import torch
    f = dfam.mixed_batch(sps, 2, 11, 6300 + 10 * sps + 2)
    B = 11
    x0, x1 = f["x0"].copy(), f["x1"].copy()
    for b in (1, 5, 3):
        x0[f["off0"][b]:f["off0"][b] + f["length"][b]] = 0
    for b in (2, 6, 3):
        x1[f["off1"][b]:f["off1"][b] + f["length"][b]] = 0
    t = ctx[sps]
    per = []
    for x, off in ((x0, f["off0"]), (x1, f["off1"])):
        ref = GpuBatch(x, off, f["length"])
        t.detect_demod_normal(ref.x, ref.off, ref.len, f["tsc"], ref.flags, ref.amp, ref.toa, ref.soft, avgpwr=ref.pwr, energy_thresh=-1.0)
        per.append(ref.results())
    v = [(r["flags"] & pkg.F_DETECT) != 0 for r in per]
    sel = dm.select(v[0], per[0]["amp"], v[1], per[1]["amp"])
    assert set(sel.tolist()) == {0, 1, 2} and sel[3] == 2 and sel[1] == 1 and sel[2] == 0
    pick = np.where(sel == 1, 1, 0)
    amp = np.where(pick == 1, per[1]["amp"], per[0]["amp"]).astype(np.complex64)
    toa = np.where(pick == 1, per[1]["toa"], per[0]["toa"]).astype(np.float32)
    want = dm.mlse_div_batch(sps, x0, f["off0"], x1, f["off1"], f["length"], f["tsc"], amp, toa, primary=pick, enable=(sel < 2).astype(np.uint8))
    try:
        for mode in (pkg.SOFT_EXACT, pkg.SOFT_TOLERANCE):
            t.set_soft_mode(mode)
            gb = GpuBatch(x0, f["off0"], f["length"], stride=160)
            flags = torch.zeros((2, B), dtype=torch.uint8, device="cuda:0"); d_amp = torch.zeros((2, B, 2), dtype=torch.float32, device="cuda:0")
            d_toa = torch.zeros((2, B), dtype=torch.float32, device="cuda:0"); pwr = torch.zeros((2, B), dtype=torch.float32, device="cuda:0")
            d_sel = torch.full((B,), 9, dtype=torch.uint8, device="cuda:0")
            chan = torch.zeros((B, 2, 5, 2), dtype=torch.float32, device="cuda:0"); win = torch.zeros(B, dtype=torch.int32, device="cuda:0")
            t.mlse_div_normal(gb.x, gb.off, dev(x1), dev(f["off1"]), gb.len, f["tsc"], flags, d_amp, d_toa, d_sel, gb.soft, avgpwr=pwr,
                              chan=chan, win=win, hard=gb.hard, energy_thresh=-1.0, soft_stride=160)
            r = gb.results()
            for a in (0, 1):
                assert flags[a].cpu().numpy().tobytes() == per[a]["flags"].tobytes(), "mode %d antenna %d: flags" % (mode, a)
                assert d_amp[a].cpu().numpy().tobytes() == per[a]["amp"].tobytes(), "mode %d antenna %d: amp" % (mode, a)
                assert d_toa[a].cpu().numpy().tobytes() == per[a]["toa"].tobytes(), "mode %d antenna %d: toa" % (mode, a)
                assert pwr[a].cpu().numpy().tobytes() == per[a]["pwr"].tobytes(), "mode %d antenna %d: avgpwr" % (mode, a)
            assert_veq(d_sel.cpu().numpy(), sel, "d_sel")
            got = dict(soft=r["soft"], hard=r["hard"], chan=chan.cpu().numpy().reshape(B, 2, 10).view(np.complex64), win=win.cpu().numpy())
            check(got, want, what="mlse_div_normal mode %d" % mode)
            assert got["win"][3] == 2 and not got["soft"][3, :148].any()
    finally:
        t.set_soft_mode(pkg.SOFT_EXACT)


@pytest.mark.parametrize("sps", [1, 4])
def test_kernel_within_the_reference_bound(ctx, sps):
    """The kernel's own soft and hard bits, windows and taps on the graded family (72 bursts at sps 1, 24 at sps 4; clean, 15 dB,
    8 dB; independent channels per antenna), graded directly by the float64 reference: no bad_soft, bad_clamp or bad_hard, and at
    most 0.5 % of the payload positions of a noise level outside the hard-bit comparison."""
    f = dfam.graded_batch(sps, per=24 if sps == 1 else 8)
    got = run_div(ctx[sps], f, stride=148)
    eq = got["win"] <= 0
    assert eq.sum() >= len(eq) - 2
    g = dref.check(got["soft"][eq], got["hard"][eq], f["want"]["y"][eq], got["win"][eq], got["chan"][eq], f["tsc"], "kernel, sps %d" % sps)
    tally = mlse_ref.Tally(mlse_family.PAYLOAD)
    tally.add(g, f["snr"][eq], f["group"][eq])
    tally.report("k_mlse_div, sps %d" % sps)
    tally.assert_cap("k_mlse_div, sps %d" % sps)


def test_refusals(pkg, ctx):
    """nsoft > 148, tsc outside 0..7, a stride below nsoft and NULL required arrays are refused (TRXSIG_EINVAL); an empty batch is a
    no-op."""
    f = dfam.mixed_batch(4, 2, 11, 6342)
    t = ctx[4]
    gb = GpuBatch(f["x0"], f["off0"][:4], f["length"][:4], stride=160)
    x1, off1 = dev(f["x1"]), dev(f["off1"][:4])
    d_amp, d_toa = dev(f["amp"][:4]), dev(f["toa"][:4])
    for kw in (dict(nsoft=149), dict(nsoft=-1), dict(tsc=8), dict(tsc=-1), dict(nsoft=148, soft_stride=147), dict(amp=None), dict(toa=None),
               dict(soft=None, soft_stride=160), dict(x1=None), dict(off1=None)):
        a = dict(tsc=2, amp=d_amp, toa=d_toa, soft=gb.soft, nsoft=148, soft_stride=160, x1=x1, off1=off1); a.update(kw)
        with pytest.raises(pkg.TrxSigError):
            t.mlse_div(gb.x, gb.off, a["x1"], a["off1"], gb.len, a["tsc"], a["amp"], a["toa"], a["soft"], nsoft=a["nsoft"], soft_stride=a["soft_stride"])
    import torch
    flags = torch.zeros((2, 4), dtype=torch.uint8, device="cuda:0"); sel = torch.zeros(4, dtype=torch.uint8, device="cuda:0")
    amp2 = torch.zeros((2, 4, 2), dtype=torch.float32, device="cuda:0"); toa2 = torch.zeros((2, 4), dtype=torch.float32, device="cuda:0")
    with pytest.raises(pkg.TrxSigError):
        t.mlse_div_normal(gb.x, gb.off, x1, off1, gb.len, 2, flags, amp2, toa2, sel, gb.soft, nsoft=149, soft_stride=160)
    with pytest.raises(pkg.TrxSigError):
        t.mlse_div_normal(gb.x, gb.off, x1, off1, gb.len, 2, flags, amp2, toa2, None, gb.soft, soft_stride=160)
    t.mlse_div(gb.x, gb.off[:0], x1, off1[:0], gb.len[:0], 2, d_amp, d_toa, gb.soft, soft_stride=160)
    torch.cuda.synchronize()
    assert np.all(gb.soft.cpu().numpy() == -1.0)
