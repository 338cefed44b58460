"""The equaliser family of tests/eq_family.py through the product library, value for value against the CPU oracle's chain
(eq_family.oracle_chain; tests/test_eq_family.py holds the oracle against the real reference on the same members):

  geometry  every maxTOA 0 .. 17 of the 52M window -- k_eq_detect<12, 26> (maxTOA <= 5 but 4), k_eq_detect52 / <9, 26, 4>
            (maxTOA 4) and k_eq_detect<36, 52> (6 .. 17) -- through trxsig_channel_estimate_batch and, energy gate off and on,
            trxsig_equalize_normal_batch; fp16 storage at maxTOA 0, 3, 5, 6, 17
  channels  designDFE alone (k_design_dfe, with and without 1 / amp), and the caller's own SNR estimate through
            trxsig_estimate_dfe_batch (design_dfe7 in a lane, design_dfe7_lanes across a wave)
  bursts    the whole chain in both variants on the amplitude ladder (energy gate off, so that every detected rung reaches
            designDFE and the equaliser, and at 10, which refuses the rungs below 2^-7), hard channels, non-finite samples and constants; the
            Transceiver/ estimate a wave per burst and a lane per burst; a hostile member moves no neighbour's result
  taps      trxsig_equalize_taps_batch_fmt with non-finite taps and amplitudes, fused (k_eq_dfe4) and as two kernels
            (k_eq_delay + k_eq_dfe2), float32 and fp16 storage: NaN where the reference has NaN and nowhere else
  and the one case with no reference: a burst too short for a wide 52M window is refused (F_BADLEN)"""
import ctypes as C

import numpy as np
import pytest

import _pkg
import eq_family as ef
import oraclebind
import synth
from test_gpu_equalize import run_eq as _run_eq
from util import assert_veq, assert_veq_nan

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def quiet_floats():
    with np.errstate(all="ignore"):                            # the members overflow and divide by zero on purpose
        yield


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def t1(pkg):
    t = pkg.TrxSig(1, 0)
    t.use_torch_stream()
    return t


@pytest.fixture(scope="module")
def oracles():
    return {False: oraclebind.Oracle(1), True: oraclebind.Oracle(1, variant52m=True)}


@pytest.fixture(scope="module")
def chains(oracles):
    """The oracle's chain for every burst of a batch, computed once per (batch, variant, threshold or SNR, maxTOA)."""
    cache = {}

    def get(bt, tsc, thr, v52, mt):
        key = (id(bt), tsc, repr(thr), type(thr).__name__, v52, mt)
        if key not in cache:
            cache[key] = (bt, [ef.oracle_chain(oracles[v52], bt.burst(i), tsc, thr, v52, mt) for i in range(len(bt))])
        return cache[key][1]
    return get


def run_eq(t, x, off, length, *a, **kw):
    """test_gpu_equalize.run_eq on copies (the family's arrays are read-only)."""
    return _run_eq(t, None if x is None else np.array(x), np.array(off), np.array(length), *a, **kw)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the family's arrays are read-only)


def cx(tensor, *shape):
    return tensor.cpu().numpy().view(np.complex64).reshape(shape)


def gpu_estimate(t, bt, tsc, v52, mt, dfe=None):
    """trxsig_channel_estimate_batch, or with dfe = dict(snr_thresh, snr_value) trxsig_estimate_dfe_batch, over a Batch."""
    import torch
    B = len(bt)
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    fl, amp, toa, co = z(B, dtype=torch.uint8), z(B, 2), z(B), z(B)
    args = (dev(bt.x.view(np.float32)), dev(bt.off), dev(bt.length), tsc, fl, amp, toa, co)
    if dfe is None:
        chan = z(B, 6, 2)
        t.channel_estimate(*args, chan, variant52m=v52, max_toa=mt)
        torch.cuda.synchronize()
        return dict(flags=fl.cpu().numpy(), amp=cx(amp, B), toa=toa.cpu().numpy(), co=co.cpu().numpy(), chan=cx(chan, B, 6))
    w, b = z(B, 7, 2), z(B, 5, 2)
    t.estimate_dfe(*args, w, b, variant52m=v52, max_toa=mt, **dfe)
    torch.cuda.synchronize()
    return dict(flags=fl.cpu().numpy(), amp=cx(amp, B), toa=toa.cpu().numpy(), co=co.cpu().numpy(), w=cx(w, B, 7), b=cx(b, B, 5))


def check_estimate(pkg, r, want, what):
    """flags, amplitude, TOA of every burst; channel response (or both filters) and offset of the detected ones."""
    for i, c in enumerate(want):
        assert bool(r["flags"][i] & pkg.F_DETECT) == c["ok"], (what, i)
        assert_veq_nan(r["amp"][i], c["amp"], "%s amp %d" % (what, i)); assert_veq_nan(r["toa"][i], c["toa"], "%s toa %d" % (what, i))
        if not c["ok"]:
            assert "chan" not in r or not r["chan"][i].any(), (what, i)
            continue
        assert r["co"][i] == c["chan_off"], (what, i)
        if "chan" in r:
            assert_veq_nan(r["chan"][i], c["chan"], "%s chan %d" % (what, i))
        else:
            assert_veq_nan(r["w"][i], c["w"], "%s w %d" % (what, i)); assert_veq_nan(r["b"][i], c["b"], "%s b %d" % (what, i))


def check_equalize(pkg, o, r, bt, want, thr, what):
    """trxsig_equalize_normal_batch's outputs against the chain; thr < 0: the energy gate is off."""
    ndet = 0
    for i, c in enumerate(want):
        e_ok = thr < 0 or o.energy_detect(bt.burst(i), 20, thr)[0]
        assert bool(r["flags"][i] & pkg.F_ENERGY) == e_ok, (what, i)
        if not e_ok:
            assert not (r["flags"][i] & pkg.F_DETECT) and not r["soft"][i].any() and not r["hard"][i].any(), (what, i)
            continue
        assert bool(r["flags"][i] & pkg.F_DETECT) == c["ok"], (what, i)
        assert_veq_nan(r["amp"][i], c["amp"], "%s amp %d" % (what, i)); assert_veq_nan(r["toa"][i], c["toa"], "%s toa %d" % (what, i))
        if not c["ok"]:
            assert not r["soft"][i].any() and not r["hard"][i].any(), (what, i)
            continue
        ndet += 1
        assert_veq_nan(r["w"][i], c["w"], "%s w %d" % (what, i)); assert_veq_nan(r["b"][i], c["b"], "%s b %d" % (what, i))
        n = min(156, len(c["soft"]))
        assert_veq_nan(r["soft"][i, :n], c["soft"][:n], "%s soft %d" % (what, i))
        assert_veq(r["hard"][i, :n], (c["soft"][:n] > 0.5).astype(np.uint8), "%s hard %d" % (what, i))
        assert not r["soft"][i, n:].any() and not r["hard"][i, n:].any(), (what, i)
    return ndet


# ---- geometry ----
@pytest.mark.parametrize("mt", ef.MAX_TOAS)
def test_geometry_every_max_toa(pkg, t1, oracles, chains, mt):
    g = ef.geometry(mt)
    assert len(g) % 64
    off = chains(g, g.tsc, 0.0, True, mt)                      # gate off: SNR = |amp|^2 / (0 + 1)
    check_estimate(pkg, gpu_estimate(t1, g, g.tsc, True, mt), off, "channel_estimate maxTOA %d" % mt)
    r = run_eq(t1, g.x, g.off, g.length, g.tsc, True, mt, -1.0)
    ndet = check_equalize(pkg, oracles[True], r, g, off, -1.0, "equalize, gate off, maxTOA %d" % mt)
    assert ndet >= len(g) // 4
    r = run_eq(t1, g.x, g.off, g.length, g.tsc, True, mt, 10.0)
    check_equalize(pkg, oracles[True], r, g, chains(g, g.tsc, 10.0, True, mt), 10.0, "equalize, gate on, maxTOA %d" % mt)


@pytest.mark.parametrize("mt", ef.FP16_MAX_TOAS)
def test_geometry_fp16_storage(pkg, t1, oracles, chains, mt):
    g = ef.geometry(mt, True)
    half = g.x.view(np.float32).reshape(-1, 2).astype(np.float16)
    assert np.array_equal(half.astype(np.float32).ravel(), g.x.view(np.float32))
    rh = run_eq(t1, None, g.off, g.length, g.tsc, True, mt, 10.0, half=half)
    rf = run_eq(t1, g.x, g.off, g.length, g.tsc, True, mt, 10.0)
    for k in rh:
        assert_veq(rh[k], rf[k], "fp16 storage vs float32 storage: %s" % k)
    ndet = check_equalize(pkg, oracles[True], rh, g, chains(g, g.tsc, 10.0, True, mt), 10.0, "fp16 storage, maxTOA %d" % mt)
    assert ndet >= len(g) // 4


def test_a_burst_shorter_than_the_52m_window_is_refused(pkg, t1):
    """The reference reads its window (samples 66 - span .. 81 + span, span = max(maxTOA, 5)) unchecked, so the family's
    ragged lengths stay at eq_family.ragged_floor and above.  The API admits 92 .. 157 at every maxTOA: what is too short
    for the window comes back as F_BADLEN alone, with amp 0, TOA 0 and zero soft bits, and moves no neighbour."""
    mt = 17
    g = ef.geometry(mt)
    floor = ef.ragged_floor(mt)
    assert floor == 99
    length = np.array(g.length)
    short = np.arange(3, len(g), 9)
    length[short] = 92 + np.arange(len(short)) % (floor - 92)                  # 92 .. 98, each more than once
    assert set(length[short]) == set(range(92, floor))
    base = run_eq(t1, g.x, g.off, g.length, g.tsc, True, mt, -1.0)
    r = run_eq(t1, g.x, g.off, length, g.tsc, True, mt, -1.0)
    assert (r["flags"][short] == pkg.F_BADLEN).all() and not r["amp"][short].any() and not r["toa"][short].any()
    assert not r["soft"][short].any() and not r["hard"][short].any()
    rest = np.setdiff1d(np.arange(len(g)), short)
    for k in r:
        assert_veq(r[k][rest], base[k][rest], "a neighbour's %s" % k)
    sub = ef.Batch(g.x, g.off, length)
    for dfe in (None, dict(snr_thresh=0.0)):
        e = gpu_estimate(t1, sub, g.tsc, True, mt, dfe=dfe)
        assert (e["flags"][short] == pkg.F_BADLEN).all() and not e["amp"][short].any() and not e["toa"][short].any()
    edge = np.array(g.length); edge[short] = floor                             # the shortest that fits is analysed
    r = run_eq(t1, g.x, g.off, edge, g.tsc, True, mt, -1.0)
    assert not (r["flags"][short] & pkg.F_BADLEN).any()


# ---- channels ----
@pytest.mark.parametrize("with_amp", [False, True], ids=["chan", "chan-over-amp"])
def test_design_dfe_on_hostile_channels(t1, oracles, with_amp):
    import torch
    c = ef.channels()
    rows = np.flatnonzero(c.use_amp == with_amp)
    n = len(rows)
    assert n >= 8 and n % 64
    w, b = torch.zeros(n, 7, 2, device="cuda"), torch.zeros(n, 5, 2, device="cuda")
    t1.design_dfe(dev(c.chan[rows].view(np.float32).reshape(n, 6, 2)), dev(c.snr[rows]), w, b,
                  amp=dev(c.amp[rows].view(np.float32).reshape(n, 2)) if with_amp else None)
    torch.cuda.synchronize()
    gw, gb = cx(w, n, 7), cx(b, n, 5)
    o = oracles[False]
    for j, i in enumerate(rows):
        ow, ob = o.design_dfe(c.scaled(o, i), float(c.snr[i]), 7)
        assert_veq_nan(gw[j], ow, "w of %s" % c.name[i]); assert_veq_nan(gb[j], ob, "b of %s" % c.name[i])


SNR_VALUES = tuple(float(np.float32(v)) for v in ef.SNRS if np.isfinite(v) and v > 0) + (37.5,)


@pytest.mark.parametrize("v52,mt", [(False, 4), (True, 4), (True, 7)], ids=["wave", "detect52", "detect-36-lags"])
def test_estimate_dfe_with_the_callers_snr(pkg, t1, chains, v52, mt):
    """snr_value > 0 is the SNR estimate itself (the facade forms it on the host), down to a denormal and up to 3e38."""
    bt = ef.bursts()
    rows = np.flatnonzero(np.isin(bt.cls, ("plain", "echoes", "maxphase")))
    sub = bt.take(rows)
    ndet = 0
    for v in SNR_VALUES:
        want = chains(sub, bt.tsc, ef.Snr(v), v52, mt)
        r = gpu_estimate(t1, sub, bt.tsc, v52, mt, dfe=dict(snr_thresh=-1.0, snr_value=v))
        check_estimate(pkg, r, want, "snr_value %r" % v)
        ndet += sum(c["ok"] for c in want)
    assert ndet >= len(SNR_VALUES) * len(sub) // 2


# ---- bursts ----
@pytest.mark.parametrize("v52", [False, True], ids=["transceiver", "52m"])
def test_bursts_through_the_whole_chain(pkg, t1, oracles, chains, v52):
    bt = ef.bursts()
    ladder = bt.cls == "ladder"
    free = chains(bt, bt.tsc, 0.0, v52, bt.max_toa)           # gate off: every detected rung of the ladder reaches designDFE and the equaliser
    r = run_eq(t1, bt.x, bt.off, bt.length, bt.tsc, v52, bt.max_toa, -1.0)
    ndet = check_equalize(pkg, oracles[v52], r, bt, free, -1.0, "bursts, gate off")
    rungs = sum(c["ok"] for c, l in zip(free, ladder) if l)
    assert ndet > len(bt) // 2 and rungs >= 75, (ndet, rungs)
    assert ((r["flags"][ladder] & pkg.F_DETECT) != 0).sum() == rungs and (r["soft"][ladder] != 0).any(axis=1).sum() == rungs
    want = chains(bt, bt.tsc, 10.0, v52, bt.max_toa)           # gate at 10: the rungs below 2^-7 come back as rows of zeros
    r = run_eq(t1, bt.x, bt.off, bt.length, bt.tsc, v52, bt.max_toa, 10.0)
    ndet = check_equalize(pkg, oracles[v52], r, bt, want, 10.0, "bursts")
    assert len(bt) // 2 < ndet < len(bt) - 20
    assert any(c["ok"] and np.isnan(c["soft"]).any() for c, h in zip(want, bt.hostile) if h)
    keep = np.flatnonzero(~bt.hostile)                         # the same batch without the hostile members
    sub = bt.take(keep)
    r2 = run_eq(t1, sub.x, sub.off, sub.length, bt.tsc, v52, bt.max_toa, 10.0)
    for k in r:
        assert_veq_nan(r2[k], r[k][keep], "a neighbour's %s moves with the hostile members" % k)


def test_bursts_estimate_a_wave_per_burst_and_a_lane_per_burst(pkg, t1, chains):
    """trxsig_estimate_dfe_batch on the Transceiver/ variant: the family alone (k_eq_estimate_wave, design_dfe7_lanes) and
    at the front of a call of more than 2,048 bursts (k_eq_detect, design_dfe7); wave, lane and oracle agree, and the
    family without its hostile members gives the others the same results."""
    bt = ef.bursts()
    want = chains(bt, bt.tsc, 12.0, False, bt.max_toa)
    dfe = dict(snr_thresh=12.0)
    wave = gpu_estimate(t1, bt, bt.tsc, False, bt.max_toa, dfe=dfe)
    check_estimate(pkg, wave, want, "a wave per burst")
    x, off, length, _ = synth.normal_batch(1, 2100 - len(bt), bt.tsc, seed=81, sigmas=(0.02, 0.3), max_delay=3.0)
    filler = ef.Batch(x, off, length)
    big = ef.pack([bt.burst(i) for i in range(len(bt))] + [filler.burst(i) for i in range(len(filler))])
    assert len(big) > 2048 and len(big) % 64
    lane = gpu_estimate(t1, big, bt.tsc, False, bt.max_toa, dfe=dfe)
    check_estimate(pkg, lane, want, "a lane per burst")
    n = len(bt)
    for k in wave:
        assert_veq_nan(lane[k][:n], wave[k], "wave against lane: %s" % k)
    keep = np.flatnonzero(~bt.hostile)
    alone = gpu_estimate(t1, bt.take(keep), bt.tsc, False, bt.max_toa, dfe=dfe)
    for k in wave:
        assert_veq_nan(alone[k], wave[k][keep], "a neighbour's %s moves with the hostile members" % k)


# ---- taps ----
@pytest.fixture(scope="module")
def taps_want(oracles):
    t = ef.taps()
    want = np.zeros((len(t), 157), np.float32)
    for i in range(len(t)):
        s = ef.equalize_member(oracles[False], t, i)
        want[i, :min(156, len(s))] = s[:156]
    return want


@pytest.mark.parametrize("fmt", [0, 1], ids=["float32", "fp16"])
@pytest.mark.parametrize("eq_tail", [1, 2], ids=["fused", "two-kernels"])
def test_equalize_with_hostile_taps(pkg, t1, taps_want, eq_tail, fmt, request):
    """Where the reference's soft bit is a NaN the library's is, and nowhere else: a feed-forward term beyond the burst is
    SKIPPED, not formed with a zero sample (0 * Inf and 0 * NaN are NaN)."""
    import torch
    t = ef.taps()
    B = len(t)
    assert B % 64 and (t.off & 1).any() and set(t.length) == set(range(92, 158))
    t1.set_tuning(eq_tail=eq_tail)
    request.addfinalizer(lambda: t1.set_tuning(eq_tail=1))
    xf = torch.from_numpy(t.x.view(np.float32).reshape(-1, 2).copy())
    dx = (xf.to(torch.float16) if fmt else xf).cuda()
    if fmt:
        assert torch.equal(dx.cpu().to(torch.float32), xf)
    soft = torch.full((B, 157), -1.0, device="cuda")
    hard = torch.full((B, 157), 9, dtype=torch.uint8, device="cuda")
    en = torch.full((B,), pkg.F_DETECT, dtype=torch.uint8, device="cuda")
    keep = [dev(t.off), dev(t.length), dev(t.amp.view(np.float32).reshape(B, 2)), dev(t.toa), dev(t.w.view(np.float32).reshape(B, 7, 2)),
            dev(t.b.view(np.float32).reshape(B, 5, 2))]
    L = t1.L
    vp, i32 = C.c_void_p, C.c_int
    L.trxsig_equalize_taps_batch_fmt.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    t1._chk(L.trxsig_equalize_taps_batch_fmt(t1.h, dx.data_ptr(), fmt, keep[0].data_ptr(), keep[1].data_ptr(), B, keep[2].data_ptr(),
                                             keep[3].data_ptr(), en.data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), soft.data_ptr(),
                                             hard.data_ptr(), 156, 157), "equalize_taps_fmt")
    torch.cuda.synchronize()
    got, gh = soft.cpu().numpy(), hard.cpu().numpy()
    bad = []
    for i in range(B):
        n = min(156, int(t.length[i]))
        if not (ef.same_with_nan(got[i, :n], taps_want[i, :n]) and np.array_equal(gh[i, :n], (taps_want[i, :n] > 0.5).astype(np.uint8))):
            bad.append(i)
    print("members that differ: %d of %d%s" % (len(bad), B, "".join("\n  %d %s len %d toa %g bad %r: NaN at %d, the reference at %d" % (
        i, t.cls[i], t.length[i], t.toa[i], t.bad[i], np.isnan(got[i, :156]).sum(), np.isnan(taps_want[i, :156]).sum()) for i in bad[:12])))
    assert not bad, (len(bad), sorted(set(t.cls[bad])))
    silent = np.flatnonzero(t.cls == "silent")
    assert (got[silent, 0] == 0.5).all() and not gh[silent, 0].any()     # an exact zero before the decision: soft 0.5, hard 0
