"""GPU parity of the interference-rejection equaliser (trxsig_mlse_irc_batch / trxsig_mlse_irc_normal_batch,
csrc/trxsig_mlse_irc.hip) against its float32 model (tests/mlse_irc_model.py): soft bits, hard bits, both tap sets, the window
word and the set (A, Bv, xr, xi) are IEEE-equal at sps 1, 2 and 4 on mixed batches of 51 bursts with an interferer on five of six
(both parities of offsets, 156- and 157-symbol lengths, every training sequence at sps 4), for B = 1, 3 and one burst more than a
workgroup takes; nsoft 100 with a stride of 160 and canaries; every optional output NULL; identities 1 and 2 against the device's
own trxsig_mlse_div_batch and trxsig_mlse_batch; the given sets that must be refused; the hostile bursts; the normal-batch call;
the refusals on a live context."""
import numpy as np
import pytest

import mlse_div_family as dfam
import mlse_div_model as dm
import mlse_family
import mlse_irc_family as ifam
import mlse_irc_model as im
import oraclebind
import mlse_run
from mlse_run import ctx, dev, pkg, run_irc  # noqa: F401  (the fixtures)
from util import GpuBatch, assert_veq

pytestmark = pytest.mark.gpu
F = np.float32


def run_one(t, x, off, length, tsc, amp, toa):
    """trxsig_mlse_batch on one antenna: dict(soft [B, 148], hard, chan [B, 5], win)."""
    import torch
    B = len(off)
    gb = GpuBatch(x, off, length, nsoft=148, stride=148)
    chan = torch.zeros((B, 5, 2), dtype=torch.float32, device="cuda:0"); win = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    t.mlse(gb.x, gb.off, gb.len, tsc, dev(amp), dev(toa), gb.soft, chan=chan, win=win, hard=gb.hard, nsoft=148, soft_stride=148)
    r = gb.results()
    return dict(soft=r["soft"], hard=r["hard"], chan=chan.cpu().numpy().reshape(B, 10).view(np.complex64), win=win.cpu().numpy())


def check(got, want, sel=None, nsoft=148, what=""):
    """mlse_run.check; the set used is among the outputs."""
    assert "cov" in got
    mlse_run.check(got, want, sel, nsoft, what)


def mixed(sps, tsc=2):
    return ifam.mixed_batch(sps, tsc, 51, 7300 + 10 * sps + tsc)


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_model_parity(ctx, sps):
    """51 bursts (seven workgroups, the last with three bursts): every output equals the model; so it does for B = 1, B = 3 (a wave
    whose second burst is missing) and B = 9 (one burst more than a workgroup takes); nsoft = 100 with a stride of 160 writes only
    that many (canaries behind the rows); a repeat gives the same bytes; every optional output may be NULL."""
    f = mixed(sps)
    want = f["want"]
    assert (want["win"] <= 0).sum() >= 45 and (f["length"] == 157 * sps).any() and (f["length"] == 156 * sps).any()
    assert len(set(((f["off0"] % 2) * 2 + f["off1"] % 2).tolist())) >= 3
    assert (np.abs(want["cov"][:, 2:]).max(axis=1) > 0.05).sum() >= 25 and f["interferer"].sum() >= 40
    got = run_irc(ctx[sps], f)
    check(got, want, what="sps %d B 51" % sps)
    for B in (1, 3, 9):
        for nsoft in ((148, 100) if B == 3 else (148,)):
            part = run_irc(ctx[sps], f, sel=np.arange(B), nsoft=nsoft)
            check(part, want, sel=np.arange(B), nsoft=nsoft, what="sps %d B %d nsoft %d" % (sps, B, nsoft))
    tail = run_irc(ctx[sps], f, sel=np.arange(40, 51), nsoft=100)
    check(tail, want, sel=np.arange(40, 51), nsoft=100, what="sps %d bursts 40..50 nsoft 100" % sps)
    again = run_irc(ctx[sps], f)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), "repeat differs: " + k
    bare = run_irc(ctx[sps], f, with_aux=False)
    assert_veq(bare["soft"][:, :148], want["soft"], "soft bits without d_cov / d_chan / d_win")
    import torch
    gb = GpuBatch(f["x0"], f["off0"], f["length"], nsoft=148, stride=160)     # ... and without d_hard, d_primary, d_enable
    ctx[sps].mlse_irc(gb.x, gb.off, dev(f["x1"]), dev(f["off1"]), gb.len, f["tsc"], dev(f["amp"]), dev(f["toa"]), gb.soft, soft_stride=160)
    torch.cuda.synchronize()
    zero = im.mlse_irc_batch(sps, f["x0"], f["off0"], f["x1"], f["off1"], f["length"], f["tsc"], f["amp"], f["toa"], y=want["y"])
    assert_veq(gb.soft.cpu().numpy()[:, :148], zero["soft"], "soft bits with every optional argument NULL")


@pytest.mark.parametrize("tsc", [0, 1, 3, 4, 5, 6, 7])
def test_every_training_sequence(ctx, tsc):
    """The other seven training sequences at sps 4 (the start states, the correlation signs and the residuals' x_m all come from
    it): 11 bursts each."""
    f = ifam.mixed_batch(4, tsc, 11, 7400 + tsc)
    check(run_irc(ctx[4], f), f["want"], what="tsc %d" % tsc)


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_identities_on_the_device(ctx, sps):
    """(1) d_cov_in = (1, 1, 0, 0): soft, hard, win and chan are the device's own trxsig_mlse_div_batch's bytes, the set that comes
    back the identity set.  (2) Antenna 1 all zeros, loading 0: they are trxsig_mlse_batch's on antenna 0."""
    f = mixed(sps)
    sel = np.arange(19)
    div = run_irc(ctx[sps], f, sel=sel, div=True)
    got = run_irc(ctx[sps], f, sel=sel, cov_in=np.tile(im.IDENTITY, (51, 1)))
    for k in ("soft", "hard", "win", "chan"):
        assert got[k].tobytes() == div[k].tobytes(), "identity set: %s differs from trxsig_mlse_div_batch" % k
    eq = div["win"] <= 0
    assert eq.sum() >= 15 and np.all(got["cov"][eq] == im.IDENTITY) and not got["cov"][~eq].any()
    est = run_irc(ctx[sps], f, sel=sel)
    assert (est["soft"] != div["soft"]).any(axis=1).sum() >= 15
    f1 = mlse_family.mixed_batch(sps, 2, 67, 4100 + sps)
    one = run_one(ctx[sps], f1["x"], f1["off"][sel], f1["length"][sel], f1["tsc"], f1["amp"][sel], f1["toa"][sel])
    base = dict(sps=sps, tsc=f1["tsc"], x0=f1["x"], off0=f1["off"][sel], length=f1["length"][sel], amp=f1["amp"][sel], toa=f1["toa"][sel],
                primary=None, x1=np.zeros_like(f1["x"]), off1=f1["off"][sel])
    got = run_irc(ctx[sps], base, stride=148, loading=0.0)
    for k in ("soft", "hard", "win"):
        assert got[k].tobytes() == one[k].tobytes(), "silent antenna: %s differs from trxsig_mlse_batch" % k
    assert got["chan"][:, 0].tobytes() == one["chan"].tobytes() and not got["chan"][:, 1].any()
    assert np.all(got["cov"][one["win"] <= 0] == im.IDENTITY)


def test_invalid_given_sets_take_the_identity_set(ctx):
    """A NaN, an infinity, 2^10, a negative diagonal, det <= 0 in d_cov_in: the identity set is taken and reported and the outputs
    are trxsig_mlse_div_batch's; valid sets beside them are used as given and equal the model."""
    f = mixed(4)
    B = 24
    sets = np.tile(im.IDENTITY, (51, 1)).astype(F)
    bad = [(np.nan, 1, 0, 0), (1, np.nan, 0, 0), (1, 1, np.nan, 0), (1, 1, 0, np.nan), (1024, 1, 0, 0), (1, 1024, 0, 0), (1, 1, -1024, 0),
           (1, 1, 0, 1024), (-1, -1, 0, 0), (1, 1, 1, 0), (1, 1, 0.8, 0.7), (0, 0, 0, 0), (np.inf, 1, 0, 0), (1, -0.5, 0, 0)]
    good = [(1023, 1023, 1000, -200), (0.5, 2, 0.3, -0.4), (2.0 ** -20, 2.0 ** -18, 0, 0), (3, 0.25, -0.5, 0.5)]
    sets[:len(bad)] = np.array(bad, F); sets[len(bad):len(bad) + len(good)] = np.array(good, F)
    sel = np.arange(B)
    want = im.mlse_irc_batch(4, f["x0"], f["off0"][sel], f["x1"], f["off1"][sel], f["length"][sel], f["tsc"], f["amp"][sel], f["toa"][sel],
                             primary=f["primary"][sel], cov_in=sets[sel], y=f["want"]["y"][sel])
    got = run_irc(ctx[4], f, sel=sel, cov_in=sets)
    check(got, want, what="given sets")
    div = run_irc(ctx[4], f, sel=sel, div=True)
    eq = div["win"] <= 0
    k = len(bad)
    assert eq[:k + len(good)].sum() >= k + len(good) - 3
    assert np.all(got["cov"][:k][eq[:k]] == im.IDENTITY) and got["soft"][:k].tobytes() == div["soft"][:k].tobytes()
    for i in range(k, k + len(good)):
        if eq[i]:
            assert np.array_equal(got["cov"][i], sets[i]) and got["soft"][i].tobytes() != div["soft"][i].tobytes()


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_hostile_bursts_on_either_antenna(ctx, sps):
    """mlse_family.hostile_batch (zeros, a NaN, an infinity, 2^31, 147 symbols, a tiny amplitude, d_enable == 0) as one antenna
    against ordinary bursts on the other, and the reverse, with d_enable and alternating d_primary: everything equals the model,
    the window words are trxsig_mlse_div_batch's (1 = fell back, 2 = skipped), the set of such a burst is zeros, and no NaN
    reaches a burst's soft bits from the other antenna's whitening."""
    h = mlse_family.hostile_batch(sps)
    g = mlse_family.mixed_batch(sps, 5, 10, 4400 + sps)
    assert np.all(h["length"] <= g["length"])
    o = oraclebind.Oracle(sps)
    primary = (np.arange(10) % 2).astype(np.uint8)
    for name, a0, a1 in (("hostile first", h, g), ("hostile second", g, h)):
        f = dict(sps=sps, tsc=5, x0=a0["x"], off0=a0["off"], x1=a1["x"], off1=a1["off"], length=h["length"], amp=h["amp"], toa=h["toa"], primary=primary)
        want = im.mlse_irc_batch(sps, f["x0"], f["off0"], f["x1"], f["off1"], f["length"], 5, f["amp"], f["toa"], primary=primary,
                                 enable=h["enable"], oracle=o)
        for b, k in enumerate(h["kind"]):
            assert (want["win"][b] == 2) if k == "disabled" else ((want["win"][b] <= 0) if k in ("plain", "zeros") else (want["win"][b] == 1)), (name, k)
            assert (want["win"][b] <= 0) or not want["cov"][b].any()
        got = run_irc(ctx[sps], f, enable=h["enable"])
        check(got, want, what="%s sps %d" % (name, sps))


@pytest.mark.parametrize("sps", [1, 4])
def test_mlse_irc_normal_batch(pkg, ctx, sps):
    """trxsig_mlse_irc_normal_batch: flags, amplitude, TOA and avgPwr of each antenna are trxsig_detect_demod_normal_batch's; d_sel is
    select() on them; the soft bits, taps, windows and sets are the model's with the selected antenna's amp and TOA and d_primary =
    d_sel, zeros (window word 2) where neither antenna detected.  Bursts 1, 5 are silent on antenna 0, 2, 6 on antenna 1, 3 on both."""
    import torch
    f = ifam.mixed_batch(sps, 2, 11, 6300 + 10 * sps + 2)
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
    want = im.mlse_irc_batch(sps, x0, f["off0"], x1, f["off1"], f["length"], f["tsc"], amp, toa, primary=pick, enable=(sel < 2).astype(np.uint8))
    gb = GpuBatch(x0, f["off0"], f["length"], stride=160)
    flags = torch.zeros((2, B), dtype=torch.uint8, device="cuda:0"); d_amp = torch.zeros((2, B, 2), dtype=torch.float32, device="cuda:0")
    d_toa = torch.zeros((2, B), dtype=torch.float32, device="cuda:0"); pwr = torch.zeros((2, B), dtype=torch.float32, device="cuda:0")
    d_sel = torch.full((B,), 9, dtype=torch.uint8, device="cuda:0")
    chan = torch.zeros((B, 2, 5, 2), dtype=torch.float32, device="cuda:0"); win = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    cov = torch.full((B, 4), -5.0, dtype=torch.float32, device="cuda:0")
    t.mlse_irc_normal(gb.x, gb.off, dev(x1), dev(f["off1"]), gb.len, f["tsc"], flags, d_amp, d_toa, d_sel, gb.soft, avgpwr=pwr, cov=cov,
                      chan=chan, win=win, hard=gb.hard, energy_thresh=-1.0, soft_stride=160)
    r = gb.results()
    for a in (0, 1):
        assert flags[a].cpu().numpy().tobytes() == per[a]["flags"].tobytes(), "antenna %d: flags" % a
        assert d_amp[a].cpu().numpy().tobytes() == per[a]["amp"].tobytes(), "antenna %d: amp" % a
        assert d_toa[a].cpu().numpy().tobytes() == per[a]["toa"].tobytes(), "antenna %d: toa" % a
        assert pwr[a].cpu().numpy().tobytes() == per[a]["pwr"].tobytes(), "antenna %d: avgpwr" % a
    assert_veq(d_sel.cpu().numpy(), sel, "d_sel")
    got = dict(soft=r["soft"], hard=r["hard"], chan=chan.cpu().numpy().reshape(B, 2, 10).view(np.complex64), win=win.cpu().numpy(),
               cov=cov.cpu().numpy())
    check(got, want, what="mlse_irc_normal")
    assert got["win"][3] == 2 and not got["soft"][3, :148].any() and not got["cov"][3].any()


def test_refusals(pkg, ctx):
    """On a live context: nsoft > 148, tsc outside 0..7, a stride below nsoft, NULL required arrays and a loading of -1, 17 or NaN
    are refused (TRXSIG_EINVAL), in both calls; the bounds 0 and 16 are accepted; an empty batch is a no-op."""
    import torch
    f = ifam.mixed_batch(4, 2, 11, 6342)
    t = ctx[4]
    gb = GpuBatch(f["x0"], f["off0"][:4], f["length"][:4], stride=160)
    x1, off1 = dev(f["x1"]), dev(f["off1"][:4])
    d_amp, d_toa = dev(f["amp"][:4]), dev(f["toa"][:4])
    for kw in (dict(nsoft=149), dict(nsoft=-1), dict(tsc=8), dict(tsc=-1), dict(nsoft=148, soft_stride=147), dict(amp=None), dict(toa=None),
               dict(soft=None, soft_stride=160), dict(x1=None), dict(off1=None), dict(loading=-1.0), dict(loading=17.0),
               dict(loading=float("nan")), dict(loading=-0.001), dict(loading=16.001)):
        a = dict(tsc=2, amp=d_amp, toa=d_toa, soft=gb.soft, nsoft=148, soft_stride=160, x1=x1, off1=off1, loading=im.LOADING); a.update(kw)
        with pytest.raises(pkg.TrxSigError):
            t.mlse_irc(gb.x, gb.off, a["x1"], a["off1"], gb.len, a["tsc"], a["amp"], a["toa"], a["soft"], loading=a["loading"], nsoft=a["nsoft"],
                       soft_stride=a["soft_stride"])
    flags = torch.zeros((2, 4), dtype=torch.uint8, device="cuda:0"); sel = torch.zeros(4, dtype=torch.uint8, device="cuda:0")
    amp2 = torch.zeros((2, 4, 2), dtype=torch.float32, device="cuda:0"); toa2 = torch.zeros((2, 4), dtype=torch.float32, device="cuda:0")
    for kw in (dict(nsoft=149), dict(loading=-1.0), dict(loading=17.0), dict(loading=float("nan")), dict(tsc=8)):
        a = dict(nsoft=148, loading=im.LOADING, tsc=2); a.update(kw)
        with pytest.raises(pkg.TrxSigError):
            t.mlse_irc_normal(gb.x, gb.off, x1, off1, gb.len, a["tsc"], flags, amp2, toa2, sel, gb.soft, loading=a["loading"], nsoft=a["nsoft"],
                              soft_stride=160)
    with pytest.raises(pkg.TrxSigError):
        t.mlse_irc_normal(gb.x, gb.off, x1, off1, gb.len, 2, flags, amp2, toa2, None, gb.soft, soft_stride=160)
    assert np.all(gb.soft.cpu().numpy() == -1.0)              # nothing refused wrote anything
    t.mlse_irc(gb.x, gb.off[:0], x1, off1[:0], gb.len[:0], 2, d_amp, d_toa, gb.soft, soft_stride=160)
    torch.cuda.synchronize()
    assert np.all(gb.soft.cpu().numpy() == -1.0)
    for loading in (0.0, 16.0):
        t.mlse_irc(gb.x, gb.off, x1, off1, gb.len, 2, d_amp, d_toa, gb.soft, loading=loading, soft_stride=160)
    torch.cuda.synchronize()
    assert np.all(gb.soft.cpu().numpy()[:, :148] >= 0.0)
