"""GPU parity of the synchronisation-burst sequence equaliser (trxsig_mlse_sch_batch, csrc/trxsig_mlse_sch.hip) against its float32
model (tests/mlse_sch_model.py): soft bits, hard bits, taps and the window word are IEEE-equal -- at sps 1, 2 and 4, on batches of
1, 3, 9 and 37 bursts, clean, noisy and multipath bursts, 156- and 157-symbol lengths, odd sample offsets (the non-wide staging
path), whole and fractional delays, TOAs on and off the 1/512 grid, and on the hostile bursts that must fall back or be skipped.
The kernel takes two bursts a wave and eight a workgroup: B = 1 leaves a wave's second half-pair of rows without a burst, B = 3
leaves the second wave half empty, B = 9 puts a workgroup one burst over, and B = 37 is four workgroups and a ragged fifth (two
waves and a half)."""
import numpy as np
import pytest

import mlse_sch_family as family
import mlse_sch_model as model
from mlse_run import check, ctx, pkg, run_sch  # noqa: F401  (the fixtures)
from util import GpuBatch, assert_veq, assert_veq_nan

pytestmark = pytest.mark.gpu
B_ALL = 37


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_model_parity(ctx, sps):
    """37 bursts: every output equals the model; a repeat is bit-equal; B = 1, 3 and 9, the batch's tail and a middle stretch give
    the batch's own values (the layout does not depend on where in a wave or a workgroup a burst lies)."""
    f = family.mixed_batch(sps, B_ALL, 6100 + sps)
    want = f["want"]
    assert (want["win"] <= 0).sum() >= 33 and len(set(want["win"].tolist())) >= 3      # the family does get equalised, in several windows
    ber = ((want["soft"][:, family.CODED] > 0.5) != f["bits"][:, family.CODED]).mean()
    assert ber < 0.05, ber                                     # ... and to the bits that were sent
    got = run_sch(ctx[sps], f)
    check(got, want, what="sps %d" % sps)
    again = run_sch(ctx[sps], f)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), "repeat differs: " + k
    for sel in (np.arange(1), np.arange(3), np.arange(9), np.arange(32, 37), np.arange(5, 22)):
        part = run_sch(ctx[sps], f, sel=sel)
        for k in got:
            assert part[k].tobytes() == got[k][sel].tobytes(), "B = %d differs from the batch: %s" % (len(sel), k)


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_hostile_bursts(ctx, sps):
    """All-zero samples, a NaN sample, an infinite one, a component of 2^31, 147 and 92 symbols, a tiny amplitude and TOA = +-4096
    fall back to the demodulator's soft bits (window word 1, taps zero); d_enable == 0, 91 symbols, a length that is no multiple of
    sps, a TOA beyond 4096 and a NaN TOA are skipped (window word 2, zeros); their neighbours are equalised, and so is the burst
    with a sample of 2^30 (its symbols stay just under the guard: the largest metrics the trellis can meet).  Where NaNs are
    expected the rule is "both NaN, or IEEE ==" (util.veq_nan)."""
    f = family.hostile_batch(sps)
    want = f["want"]
    kind = f["kind"]
    skipped = {"disabled", "len_91", "toa_past", "toa_nan"} | ({"len_odd"} if sps > 1 else set())
    for b, k in enumerate(kind):
        word = want["win"][b]
        if k in skipped:
            assert word == 2, (k, word)
        elif k == "plain" or (k == "len_odd" and sps == 1):
            assert word <= 0, (k, word)
        elif k == "p30":                                        # 2^30 before the delay filter: just under the guard after it, and equalised
            assert word <= 1 and np.abs(want["y"][b].view(np.float32)).max() > 2.0 ** 29, (k, word)
        else:
            assert word == 1, (k, word)
    assert np.isnan(want["soft"][kind.index("nan")]).any()
    got = run_sch(ctx[sps], f, enable=f["enable"])
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
        elif want["win"][b] <= 0:                               # an equalised burst keeps the demodulator's bits on the training sequence
            assert_veq(got["soft"][b, 42:106], dem[b, 42:106], "burst %d, the extended training sequence" % b)
            assert np.all(got["soft"][b, [0, 1, 2, 145, 146, 147]] == 0.0), "burst %d: the tail bits are not exactly 0" % b


def test_nsoft_and_null_outputs(ctx):
    """nsoft in {148, 145, 106, 107, 42, 41, 3, 0} with stride 160 writes only that many; d_chan, d_win and d_hard may be NULL;
    d_enable skips."""
    f = family.mixed_batch(4, B_ALL, 6104)
    sel = np.arange(9)
    for nsoft in (148, 145, 106, 107, 42, 41, 3, 0):
        got = run_sch(ctx[4], f, sel=sel, nsoft=nsoft, stride=160)
        check(got, f["want"], sel=sel, nsoft=nsoft, what="nsoft %d" % nsoft)
    got = run_sch(ctx[4], f, sel=sel, with_aux=False)
    assert_veq(got["soft"][:, :148], f["want"]["soft"][sel], "soft bits without d_chan / d_win")
    got = run_sch(ctx[4], f, sel=sel, with_hard=False)
    assert_veq(got["soft"][:, :148], f["want"]["soft"][sel], "soft bits without d_hard")
    assert np.all(got["hard"] == 255), "d_hard == NULL, and hard bits were written somewhere"
    enable = (np.arange(B_ALL) % 3 != 1).astype(np.uint8)
    want = model.sch_batch(4, f["x"], f["off"], f["length"], f["amp"], f["toa"], enable=enable)
    assert (want["win"] == 2).sum() == int((enable == 0).sum())
    check(run_sch(ctx[4], f, enable=enable), want, what="d_enable")


def test_soft_mode_has_no_bearing(pkg, ctx):
    f = family.mixed_batch(4, B_ALL, 6104)
    sel = np.arange(9)
    ctx[4].set_soft_mode(pkg.SOFT_TOLERANCE)
    try:
        got = run_sch(ctx[4], f, sel=sel)
    finally:
        ctx[4].set_soft_mode(pkg.SOFT_EXACT)
    check(got, f["want"], sel=sel, what="tolerance mode")


def test_refusals(pkg, ctx):
    """nsoft > 148, a stride below nsoft and NULL arrays are refused (TRXSIG_EINVAL); an empty batch is a no-op."""
    import torch
    f = family.mixed_batch(4, B_ALL, 6104)
    t = ctx[4]
    gb = GpuBatch(f["x"], f["off"][:4], f["length"][:4], stride=160)
    d_amp = torch.from_numpy(f["amp"][:4].view(np.float32).copy()).cuda(); d_toa = torch.from_numpy(f["toa"][:4].copy()).cuda()
    for kw in (dict(nsoft=149), dict(nsoft=-1), dict(nsoft=148, soft_stride=147), dict(amp=None), dict(toa=None), dict(soft=None, soft_stride=160)):
        a = dict(amp=d_amp, toa=d_toa, soft=gb.soft, nsoft=148, soft_stride=160); a.update(kw)
        with pytest.raises(pkg.TrxSigError):
            t.mlse_sch(gb.x, gb.off, gb.len, a["amp"], a["toa"], a["soft"], nsoft=a["nsoft"], soft_stride=a["soft_stride"])
    with pytest.raises(pkg.TrxSigError):
        t.mlse_sch(None, gb.off, gb.len, d_amp, d_toa, gb.soft, soft_stride=160)
    t.mlse_sch(gb.x, gb.off[:0], gb.len[:0], d_amp, d_toa, gb.soft, soft_stride=160)
    torch.cuda.synchronize()
    assert np.all(gb.soft.cpu().numpy() == -1.0)
