"""GPU parity, config 5: the Transceiver52M pullRadioVector TSC leg at sps=1 -- energyDetect (stride 4),
windowed analyzeTrafficBurst with channel estimate, designDFE(Nf=7), equalizeBurst -- and the
Transceiver/ (full-window) variant.  Golden vectors of the real reference + CPU oracle.  Value-exact."""
import numpy as np
import pytest

import _pkg
import oraclebind
from util import assert_veq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    return _pkg.load()


@pytest.fixture(scope="module")
def t1(pkg):
    t = pkg.TrxSig(1, 0)
    t.use_torch_stream()
    return t


def run_eq(t, x, off, length, tsc, variant52m, max_toa, thr, nsoft=156, half=None):
    """half: the batch as float16 I/Q pairs [n, 2] -- read by the kernels directly (trxsig_equalize_normal_batch_fmt)."""
    import torch
    B = len(off)
    dev = "cuda"
    if half is not None:
        d = dict(flags=torch.zeros(B, dtype=torch.uint8, device=dev), amp=torch.zeros(B, 2, device=dev),
                 toa=torch.zeros(B, device=dev), w=torch.zeros(B, 7, 2, device=dev), b=torch.zeros(B, 5, 2, device=dev),
                 soft=torch.zeros(B, 157, device=dev), hard=torch.zeros(B, 157, dtype=torch.uint8, device=dev))
        t.equalize_normal(torch.from_numpy(np.ascontiguousarray(half).view(np.int16).copy()).cuda(),
                          torch.from_numpy(np.ascontiguousarray(off, np.int32)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(length, np.int32)).cuda(), tsc, d["flags"], d["amp"],
                          d["toa"], d["soft"], w=d["w"], b=d["b"], hard=d["hard"], energy_thresh=thr,
                          variant52m=variant52m, max_toa=max_toa, nsoft=nsoft, soft_stride=157, fp16=True)
        torch.cuda.synchronize()
        r = {k: v.cpu().numpy() for k, v in d.items()}
        r["amp"] = r["amp"].view(np.complex64).ravel()
        r["w"] = r["w"].view(np.complex64).reshape(B, 7); r["b"] = r["b"].view(np.complex64).reshape(B, 5)
        return r
    d = dict(flags=torch.zeros(B, dtype=torch.uint8, device=dev), amp=torch.zeros(B, 2, device=dev),
             toa=torch.zeros(B, device=dev), w=torch.zeros(B, 7, 2, device=dev), b=torch.zeros(B, 5, 2, device=dev),
             soft=torch.zeros(B, 157, device=dev), hard=torch.zeros(B, 157, dtype=torch.uint8, device=dev))
    t.equalize_normal(torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda(),
                      torch.from_numpy(np.ascontiguousarray(off, np.int32)).cuda(),
                      torch.from_numpy(np.ascontiguousarray(length, np.int32)).cuda(), tsc, d["flags"], d["amp"],
                      d["toa"], d["soft"], w=d["w"], b=d["b"], hard=d["hard"], energy_thresh=thr,
                      variant52m=variant52m, max_toa=max_toa, nsoft=nsoft, soft_stride=157)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in d.items()}
    r["amp"] = r["amp"].view(np.complex64).ravel()
    r["w"] = r["w"].view(np.complex64).reshape(B, 7); r["b"] = r["b"].view(np.complex64).reshape(B, 5)
    return r


def test_golden_dfe_52m(pkg, t1, golden):
    g = golden("dfe_52m_sps1.npz")
    for tsc in range(8):
        sel = np.flatnonzero(g["tsc"] == tsc)
        r = run_eq(t1, g["x"], g["off"][sel], g["len"][sel], tsc, True, 4, float(g["energy_thresh"]))
        assert_veq((r["flags"] & pkg.F_ENERGY) != 0, g["energy_ok"][sel].astype(bool), "energy")
        det = (r["flags"] & pkg.F_DETECT) != 0
        assert_veq(det, g["ok"][sel].astype(bool) & g["energy_ok"][sel].astype(bool), "detect")
        for j, i in enumerate(sel):
            if not det[j]:
                continue
            assert r["amp"][j] == g["amp"][i] and r["toa"][j] == g["toa"][i], (i, r["amp"][j], g["amp"][i])
            assert_veq(r["w"][j], g["w"][i], "w %d" % i); assert_veq(r["b"][j], g["b"][i], "b %d" % i)
            n = int(g["len"][i])
            assert_veq(r["soft"][j, :n - 1 if n == 157 else n][:156], g["soft"][i, :156][:n], "DFE soft %d" % i)


@pytest.mark.parametrize("variant52m,tail", [(True, None), (False, None), (True, "2")])
def test_random_dfe_vs_oracle(pkg, t1, variant52m, tail, request):
    # tail "2": scaleVector + delayVector + equalizeBurst as two kernels through the scratch rows (k_eq_delay + k_eq_dfe2) instead of the fused
    # k_eq_dfe4 (trxsig_set_tuning(TRXSIG_TUNE_EQ_TAIL): library-wide, read at every call)
    if tail:
        t1.set_tuning(eq_tail=int(tail))
        request.addfinalizer(lambda: t1.set_tuning(eq_tail=1))
    rng = np.random.default_rng(99 + variant52m)
    o = oraclebind.Oracle(1, variant52m=variant52m)
    from openbts_ttsou_amd import synth
    B, tsc, thr = 512, 6, 10.0
    x, off, length, meta = synth.normal_batch(1, B, tsc, seed=17 + variant52m, sigmas=(0.02, 0.1), max_delay=1.0)
    # two-path channel on odd bursts
    for i in range(1, B, 2):
        s = x[off[i]:off[i] + length[i]]
        s[1:] = s[1:] + np.complex64(0.4 + 0.2j) * s[:-1].copy()
    mt = 4
    r = run_eq(t1, x, off, length, tsc, variant52m, mt, thr)
    nerr = 0
    for i in range(B):
        s = x[off[i]:off[i] + length[i]]
        ok_e, _ = o.energy_detect(s, 20, thr)
        assert bool(r["flags"][i] & pkg.F_ENERGY) == ok_e
        if not ok_e:
            continue
        a = o.analyze_traffic(s, tsc, 3.0, req_chan=True, max_toa=mt)
        assert bool(r["flags"][i] & pkg.F_DETECT) == a["ok"], i
        assert r["amp"][i] == a["amp"] and r["toa"][i] == a["toa"], (i, r["amp"][i], a["amp"], r["toa"][i], a["toa"])
        if not a["ok"]:
            continue
        am = a["amp"]
        n2 = np.float32(np.float32(am.imag * am.imag) + np.float32(am.real * am.real))
        inv = complex(np.float32(am.real / n2), np.float32(-am.imag / n2))
        snr = np.float32(np.float64(n2) / (np.float64(np.float32(thr * thr)) + 1.0))
        w, b = o.design_dfe(o.scale_vector(a["chan"], inv), float(snr), 7)
        assert_veq(r["w"][i], w, "w %d" % i); assert_veq(r["b"][i], b, "b %d" % i)
        soft = o.equalize(o.scale_vector(s, inv), np.float32(a["toa"] - a["chan_off"]), w, b)
        assert_veq(r["soft"][i, :156], soft[:156], "soft %d" % i)
        nerr += int(((soft[:148] > 0.5) != meta["bits"][i]).sum())
    assert nerr < 0.02 * B * 148


def test_config5_fp16_samples(pkg, t1):
    """BASELINE config 5: bursts stored as fp16 I/Q (values restricted to fp16-exact integers, |v| <= 2048)
    and read AS fp16 by the 52M equaliser leg's kernels (trxsig_equalize_normal_batch_fmt: no float32 copy of the batch,
    no conversion pass).  Widening is exact, so everything must equal the float32 call on the same numbers and, burst by
    burst for ALL bursts, the 52M CPU oracle: flags, amplitude, TOA, both DFE filters and every soft bit.  Odd sample
    offsets (the 4-byte load path) and ragged lengths included."""
    import torch
    from openbts_ttsou_amd import synth
    B, tsc, thr, mt = 384, 3, 10.0, 4
    x, off, length, meta = synth.normal_batch(1, B, tsc, seed=555, sigmas=(0.02, 0.1, 0.6), max_delay=1.0)
    for i in range(1, B, 2):                                            # {1, 0.4+0.2j, 0} multipath on odd bursts
        s = x[off[i]:off[i] + length[i]]
        s[1:] = s[1:] + np.complex64(0.4 + 0.2j) * s[:-1].copy()
    for i in range(5, B, 11):                                           # silent slots: the energy gate must hold them
        x[off[i]:off[i] + length[i]] *= np.float32(1e-3)
    scale = 2000.0 / np.abs(x.view(np.float32)).max()
    q = np.clip(np.rint(x.view(np.float32) * scale), -2048, 2048).astype(np.float16)     # fp16-exact integers
    xq = q.astype(np.float32).view(np.complex64)
    assert np.array_equal(xq.view(np.float32), q.astype(np.float32))
    # repack with a one-sample gap after every third burst: odd offsets take the narrow load path
    gaps = (np.arange(B) % 3 == 2).astype(np.int64)
    off2 = (off.astype(np.int64) + np.concatenate([[0], np.cumsum(gaps)[:-1]])).astype(np.int32)
    q2 = np.zeros((int(off2[-1] + length[-1]) + 1, 2), np.float16)
    for i in range(B):
        q2[off2[i]:off2[i] + length[i]] = q.reshape(-1, 2)[off[i]:off[i] + length[i]]
    assert (off2 & 1).any()
    xq2 = q2.astype(np.float32).view(np.complex64).ravel()
    r = run_eq(t1, None, off2, length, tsc, True, mt, thr, half=q2)
    rf = run_eq(t1, xq2, off2, length, tsc, True, mt, thr)
    for k in r:
        assert_veq(r[k], rf[k], "fp16 storage vs float32 storage: %s" % k)
    # the float32 pipeline with an explicit widening pass (trxsig_unpack_half) is the same thing in two steps
    d_half = torch.from_numpy(q2.view(np.int16).copy()).cuda()
    d_f32 = torch.zeros(len(xq2), 2, device="cuda")
    t1.unpack_half(d_half, len(xq2), d_f32)
    torch.cuda.synchronize()
    assert np.array_equal(d_f32.cpu().numpy().ravel(), q2.astype(np.float32).ravel())
    o = oraclebind.Oracle(1, variant52m=True)
    ndet = nerr = ngate = 0
    for i in range(B):
        s = xq2[off2[i]:off2[i] + length[i]]
        ok_e, _ = o.energy_detect(s, 20, thr)
        assert bool(r["flags"][i] & pkg.F_ENERGY) == ok_e, i
        if not ok_e:
            ngate += 1
            assert not (r["flags"][i] & pkg.F_DETECT) and not r["soft"][i].any()
            continue
        a = o.analyze_traffic(s, tsc, 3.0, req_chan=True, max_toa=mt)
        assert bool(r["flags"][i] & pkg.F_DETECT) == a["ok"], i
        assert r["amp"][i] == a["amp"] and r["toa"][i] == a["toa"], i
        if not a["ok"]:
            continue
        ndet += 1
        am = a["amp"]
        n2 = np.float32(np.float32(am.imag * am.imag) + np.float32(am.real * am.real))
        inv = complex(np.float32(am.real / n2), np.float32(-am.imag / n2))
        snr = np.float32(np.float64(n2) / (np.float64(np.float32(thr * thr)) + 1.0))
        w, b = o.design_dfe(o.scale_vector(a["chan"], inv), float(snr), 7)
        assert_veq(r["w"][i], w, "w %d" % i); assert_veq(r["b"][i], b, "b %d" % i)
        soft = o.equalize(o.scale_vector(s, inv), np.float32(a["toa"] - a["chan_off"]), w, b)
        assert_veq(r["soft"][i, :156], soft[:156], "soft %d" % i)
        assert_veq(r["hard"][i, :156], (soft[:156] > 0.5).astype(np.uint8), "hard %d" % i)
        if meta["sigma"][i] <= 0.1:
            nerr += int(((soft[:148] > 0.5) != meta["bits"][i]).sum())
    assert ndet > B // 2 and ngate >= B // 12 and nerr < 0.02 * ndet * 148


@pytest.mark.parametrize("variant52m", [True, False])
def test_channel_estimate_and_design_dfe_on_their_own(pkg, t1, variant52m):
    """analyzeTrafficBurst(requestChannel) and designDFE as separate calls (the facade's route, sigProcLib.h:277-285,
    365-369): channel response, offset and both filters value-exact against the oracle's."""
    import torch
    from openbts_ttsou_amd import synth
    o = oraclebind.Oracle(1, variant52m=variant52m)
    B, tsc, mt = 384, 6, 4
    x, off, length, meta = synth.normal_batch(1, B, tsc, seed=4711 + variant52m, sigmas=(0.02, 0.1, 1.5), max_delay=1.0)
    for i in range(1, B, 2):
        s = x[off[i]:off[i] + length[i]]
        s[1:] = s[1:] + np.complex64(0.4 + 0.2j) * s[:-1].copy()
    dev = "cuda"
    dx = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    doff = torch.from_numpy(off.astype(np.int32)).cuda(); dlen = torch.from_numpy(length.astype(np.int32)).cuda()
    flags = torch.zeros(B, dtype=torch.uint8, device=dev); amp = torch.zeros(B, 2, device=dev); toa = torch.zeros(B, device=dev)
    choff = torch.zeros(B, device=dev); chan = torch.zeros(B, 6, 2, device=dev)
    t1.channel_estimate(dx, doff, dlen, tsc, flags, amp, toa, choff, chan, variant52m=variant52m, max_toa=mt)
    snr = torch.full((B,), 37.5, device=dev)
    w = torch.zeros(B, 7, 2, device=dev); b = torch.zeros(B, 5, 2, device=dev)
    t1.design_dfe(chan, snr, w, b, amp=amp)
    torch.cuda.synchronize()
    fl = flags.cpu().numpy(); ch = chan.cpu().numpy().view(np.complex64).reshape(B, 6); co = choff.cpu().numpy()
    am = amp.cpu().numpy().view(np.complex64).ravel(); wv = w.cpu().numpy().view(np.complex64).reshape(B, 7)
    bv = b.cpu().numpy().view(np.complex64).reshape(B, 5)
    ndet = 0
    for i in range(B):
        a = o.analyze_traffic(x[off[i]:off[i] + length[i]], tsc, 3.0, req_chan=True, max_toa=mt)
        assert bool(fl[i] & pkg.F_DETECT) == a["ok"], i
        assert am[i] == a["amp"] and toa[i].item() == a["toa"], i
        if not a["ok"]:
            assert not ch[i].any()
            continue
        ndet += 1
        assert_veq(ch[i], a["chan"], "chan %d" % i); assert co[i] == a["chan_off"]
        n2 = np.float32(np.float32(a["amp"].imag * a["amp"].imag) + np.float32(a["amp"].real * a["amp"].real))
        inv = complex(np.float32(a["amp"].real / n2), np.float32(-a["amp"].imag / n2))
        ow, ob = o.design_dfe(o.scale_vector(a["chan"], inv), 37.5, 7)
        assert_veq(wv[i], ow, "w %d" % i); assert_veq(bv[i], ob, "b %d" % i)
    assert ndet > B // 2


@pytest.mark.parametrize("tsc", [0, 5, 7])
def test_channel_estimate_52m_every_peak_position(pkg, t1, tsc):
    """The 52M window with maxTOA = 4 runs in its own kernel (k_eq_detect52: nine lags in registers, interpolatePoint over
    lags 0..7 at every point of the bisection): bursts that arrive up to five symbols early or late (the peak on every lag,
    TOAs outside the window), pure noise (peaks anywhere, most not detected), single impulses (equal powers on every lag:
    peakDetect's "else break" and the argmax's first-wins rule), all-zero bursts (no peak at all: maxIndex = -1) and ragged
    lengths -- flags, amplitude, TOA, channel response and offset value for value against the oracle, energy gate off."""
    import torch
    from openbts_ttsou_amd import synth
    o = oraclebind.Oracle(1, variant52m=True)
    rng = np.random.default_rng(52 + tsc)
    B, mt = 1000, 4                                              # (not a multiple of the kernel's 256 bursts per workgroup)
    x, off, length, meta = synth.normal_batch(1, B, tsc, seed=9000 + tsc, sigmas=(0.02, 0.3), max_delay=5.2)
    x = x.copy()
    kinds = rng.integers(0, 10, B)
    for i in range(B):
        s = x[off[i]:off[i] + length[i]]
        if kinds[i] in (0, 1, 2):                                # noise only
            s[:] = (rng.standard_normal(len(s)) + 1j * rng.standard_normal(len(s))).astype(np.complex64) * np.float32(100.0)
        elif kinds[i] == 3:                                      # one impulse inside the correlation window
            s[:] = 0
            s[int(rng.integers(58, 90))] = np.complex64(complex(rng.integers(1, 50), rng.integers(-50, 50)))
        elif kinds[i] == 4 and i % 3 == 0:                       # nothing at all
            s[:] = 0
    length = length.copy()
    cut = np.flatnonzero(kinds == 5)
    length[cut] = rng.integers(92, 157, len(cut))                # ragged (the window always fits: 87 samples)
    dev = "cuda"
    dx = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    doff = torch.from_numpy(off.astype(np.int32)).cuda(); dlen = torch.from_numpy(length.astype(np.int32)).cuda()
    flags = torch.zeros(B, dtype=torch.uint8, device=dev); amp = torch.zeros(B, 2, device=dev); toa = torch.zeros(B, device=dev)
    choff = torch.zeros(B, device=dev); chan = torch.zeros(B, 6, 2, device=dev)
    t1.channel_estimate(dx, doff, dlen, tsc, flags, amp, toa, choff, chan, variant52m=True, max_toa=mt)
    torch.cuda.synchronize()
    fl = flags.cpu().numpy(); ch = chan.cpu().numpy().view(np.complex64).reshape(B, 6); co = choff.cpu().numpy()
    am = amp.cpu().numpy().view(np.complex64).ravel(); tv = toa.cpu().numpy()
    ndet, peaks = 0, set()
    for i in range(B):
        a = o.analyze_traffic(x[off[i]:off[i] + length[i]], tsc, 3.0, req_chan=True, max_toa=mt)
        assert bool(fl[i] & pkg.F_DETECT) == a["ok"], (i, kinds[i])
        assert am[i] == a["amp"] and tv[i] == a["toa"], (i, kinds[i], am[i], a["amp"], tv[i], a["toa"])
        if not a["ok"]:
            assert not ch[i].any()
            continue
        ndet += 1
        peaks.add(int(np.rint(a["toa"])))
        assert_veq(ch[i], a["chan"], "chan %d" % i); assert co[i] == a["chan_off"], i
    assert ndet > B // 4 and len(peaks) >= 8, (ndet, sorted(peaks))


@pytest.mark.parametrize("tsc", [1, 6])
def test_estimate_dfe_a_wave_per_burst_and_a_lane_per_burst(pkg, t1, tsc):
    """trxsig_estimate_dfe_batch on the Transceiver/ variant (the 36-lag window) takes a wave per burst for small calls and marked
    subsets (k_eq_estimate_wave: speculated bisection, designDFE across lanes) and a lane per burst for large ones (k_eq_detect): the
    same bursts through both -- a call of 700 and the same 700 inside a call of 2,900 -- must agree value for value with each other
    and with the oracle: flags, amplitude, TOA, channel offset and both DFE filters.  Early / late bursts, noise, an impulse, silence."""
    import torch
    import synth
    o = oraclebind.Oracle(1, variant52m=False)
    rng = np.random.default_rng(77 + tsc)
    Bs, Bl = 700, 2900
    x, off, length, meta = synth.normal_batch(1, Bl, tsc, seed=300 + tsc, sigmas=(0.02, 0.3), max_delay=6.0)
    x = x.copy()
    for i in range(0, Bs, 7):
        s = x[off[i]:off[i] + length[i]]
        kind = (i // 7) % 4
        if kind == 0:
            s[:] = (rng.standard_normal(len(s)) + 1j * rng.standard_normal(len(s))).astype(np.complex64) * np.float32(50.0)
        elif kind == 1:
            s[:] = 0; s[int(rng.integers(56, 92))] = np.complex64(complex(rng.integers(1, 50), rng.integers(-50, 50)))
        elif kind == 2 and i % 3 == 0:
            s[:] = 0
    dev = "cuda"
    dx = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    out = {}
    for B in (Bs, Bl):
        doff = torch.from_numpy(off[:B].astype(np.int32)).cuda(); dlen = torch.from_numpy(length[:B].astype(np.int32)).cuda()
        r = dict(flags=torch.zeros(B, dtype=torch.uint8, device=dev), amp=torch.zeros(B, 2, device=dev), toa=torch.zeros(B, device=dev),
                 co=torch.zeros(B, device=dev), w=torch.zeros(B, 7, 2, device=dev), b=torch.zeros(B, 5, 2, device=dev))
        t1.estimate_dfe(dx, doff, dlen, tsc, r["flags"], r["amp"], r["toa"], r["co"], r["w"], r["b"], snr_thresh=12.0)
        torch.cuda.synchronize()
        out[B] = dict(fl=r["flags"].cpu().numpy(), am=r["amp"].cpu().numpy().view(np.complex64).ravel(), toa=r["toa"].cpu().numpy(),
                      co=r["co"].cpu().numpy(), w=r["w"].cpu().numpy().view(np.complex64).reshape(B, 7),
                      b=r["b"].cpu().numpy().view(np.complex64).reshape(B, 5))
    a, c = out[Bs], out[Bl]
    ndet = 0
    for i in range(Bs):
        ref = o.analyze_traffic(x[off[i]:off[i] + length[i]], tsc, 3.0, req_chan=True, max_toa=4)
        for r in (a, c):
            assert bool(r["fl"][i] & pkg.F_DETECT) == ref["ok"], i
            assert r["am"][i] == ref["amp"] and r["toa"][i] == ref["toa"], (i, r["am"][i], ref["amp"], r["toa"][i], ref["toa"])
        if not ref["ok"]:
            continue
        ndet += 1
        am = ref["amp"]
        n2 = np.float32(np.float32(am.imag * am.imag) + np.float32(am.real * am.real))
        inv = complex(np.float32(am.real / n2), np.float32(-am.imag / n2))
        snr = np.float32(np.float64(n2) / (np.float64(np.float32(12.0 * 12.0)) + 1.0))
        ow, ob = o.design_dfe(o.scale_vector(ref["chan"], inv), float(snr), 7)
        for r in (a, c):
            assert r["co"][i] == ref["chan_off"], i
            assert_veq(r["w"][i], ow, "w %d" % i); assert_veq(r["b"][i], ob, "b %d" % i)
    assert ndet > Bs // 2


def test_equalize_taps_rejected_burst_is_not_equalised_from_stale_scratch(pkg, t1):
    """trxsig_equalize_taps_batch with caller-supplied flags: a burst the delay kernel refuses (bad length, |TOA| > 4096 or
    NaN) must come back as zeros even when its scratch row still holds an earlier call's burst."""
    import torch
    from openbts_ttsou_amd import synth
    B, tsc = 64, 2
    x, off, length, meta = synth.normal_batch(1, B, tsc, seed=8, sigmas=(0.02,), max_delay=0.5)
    dev = "cuda"
    dx = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    doff = torch.from_numpy(off.astype(np.int32)).cuda(); dlen = torch.from_numpy(length.astype(np.int32)).cuda()
    amp = torch.ones(B, 2, device=dev); amp[:, 1] = 0
    w = torch.zeros(B, 7, 2, device=dev); w[:, 0, 0] = 1.0
    b = torch.zeros(B, 5, 2, device=dev)
    en = torch.full((B,), pkg.F_DETECT, dtype=torch.uint8, device=dev)
    soft = torch.full((B, 157), -1.0, device=dev)
    toa = torch.zeros(B, device=dev)
    L = t1.L
    L.trxsig_equalize_taps_batch.argtypes = [__import__("ctypes").c_void_p] * 4 + [__import__("ctypes").c_int] + [__import__("ctypes").c_void_p] * 7 + \
        [__import__("ctypes").c_int] * 2
    def call():
        t1._chk(L.trxsig_equalize_taps_batch(t1.h, dx.data_ptr(), doff.data_ptr(), dlen.data_ptr(), B, amp.data_ptr(), toa.data_ptr(),
                                             en.data_ptr(), w.data_ptr(), b.data_ptr(), soft.data_ptr(), None, 156, 157), "equalize_taps")
        torch.cuda.synchronize()
        return soft.cpu().numpy().copy()
    first = call()
    assert (first[:, :148] != 0).any(axis=1).all()                 # every burst produced soft bits; the scratch rows are now warm
    toa[3] = float("nan"); toa[5] = 5000.0; toa[7] = -1e9
    dlen2 = dlen.clone(); dlen2[9] = 40
    dlen, keep = dlen2, dlen
    soft.fill_(-1.0)
    second = call()
    for i in (3, 5, 7, 9):
        assert not second[i, :156].any(), i
    ok = [i for i in range(B) if i not in (3, 5, 7, 9)]
    assert np.array_equal(second[ok], first[ok])


@pytest.mark.parametrize("eq_tail", [1, 2], ids=["fused", "two-kernels"])
def test_delay_and_equalize_with_arbitrary_toa_lengths_and_taps(pkg, t1, eq_tail, request):
    """trxsig_equalize_taps_batch -- the fused k_eq_dfe4 (eq_tail 1, the default) and k_eq_delay + k_eq_dfe2 through the
    scratch rows (eq_tail 2: trxsig_set_tuning(TRXSIG_TUNE_EQ_TAIL), library-wide, restored when the test ends) -- on
    inputs analyzeTrafficBurst would never produce: every length from 92 to 157 at ragged odd offsets, TOAs on the 1/512 grid, off it (table sinc computed in the kernel), within
    1e-2 of an integer (delayVector's copy branch), integer shifts of tens and hundreds of samples in both directions (the
    burst leaves the staging row partly or wholly), random amplitudes and random feed-forward / feedback taps; float32 and
    fp16 storage.  Every soft bit value-exact against scaleVector + equalizeBurst of the oracle."""
    import ctypes as C
    import torch
    t1.set_tuning(eq_tail=eq_tail)
    request.addfinalizer(lambda: t1.set_tuning(eq_tail=1))
    rng = np.random.default_rng(2024)
    o = oraclebind.Oracle(1)
    B = 528
    lens = np.concatenate([np.arange(92, 158), rng.integers(92, 158, B - 66)]).astype(np.int32)
    gaps = rng.integers(0, 4, B)
    off = np.zeros(B, np.int32)
    pos = 1
    for i in range(B):
        off[i] = pos; pos += int(lens[i]) + int(gaps[i])
    xq = rng.integers(-1500, 1501, (pos + 8, 2)).astype(np.float32)          # fp16-exact integers: both storages see the same values
    toa = np.empty(B, np.float32)
    kinds = rng.integers(0, 6, B)
    for i in range(B):
        k = kinds[i]
        if k == 0: toa[i] = rng.integers(-8 * 512, 8 * 512) / 512.0                       # on the grid
        elif k == 1: toa[i] = np.float32(rng.uniform(-9, 9))                             # off the grid
        elif k == 2: toa[i] = np.float32(rng.integers(-6, 7) + rng.choice([-1, 1]) * rng.uniform(0, 9e-3))   # copy branch
        elif k == 3: toa[i] = np.float32(rng.integers(-40, 41) + rng.integers(0, 512) / 512.0)             # tens of samples
        elif k == 4: toa[i] = np.float32(rng.choice([-300.25, -157.0, -100.5, 99.75, 156.5, 2000.125, 4096.0, -4096.0]))
        else: toa[i] = 0.0
    toa[5:9] = np.float32([1e-9, 3e-8, -1e-9, 2.0 + 1e-7])   # tiny positive TOA: the delay's fraction rounds to exactly 1.0
    amp = (rng.uniform(0.2, 40, B) * np.exp(2j * np.pi * rng.uniform(0, 1, B))).astype(np.complex64)
    w = (rng.normal(0, 0.4, (B, 7)) + 1j * rng.normal(0, 0.4, (B, 7))).astype(np.complex64)
    b = (rng.normal(0, 0.2, (B, 5)) + 1j * rng.normal(0, 0.2, (B, 5))).astype(np.complex64)
    dev = "cuda"
    doff = torch.from_numpy(off).cuda(); dlen = torch.from_numpy(lens).cuda()
    damp = torch.from_numpy(amp.view(np.float32).reshape(B, 2)).cuda(); dtoa = torch.from_numpy(toa).cuda()
    dw = torch.from_numpy(w.view(np.float32).reshape(B, 7, 2)).cuda(); db = torch.from_numpy(b.view(np.float32).reshape(B, 5, 2)).cuda()
    en = torch.full((B,), pkg.F_DETECT, dtype=torch.uint8, device=dev)
    L = t1.L
    vp, i32 = C.c_void_p, C.c_int
    L.trxsig_equalize_taps_batch_fmt.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    want = np.zeros((B, 157), np.float32)
    xc = xq.view(np.complex64).ravel()
    for i in range(B):
        s = xc[off[i]:off[i] + lens[i]]
        a = amp[i]
        n2 = np.float32(np.float32(a.imag * a.imag) + np.float32(a.real * a.real))
        inv = complex(np.float32(a.real / n2), np.float32(-a.imag / n2))
        soft = o.equalize(o.scale_vector(s, inv), np.float32(toa[i]), w[i], b[i])
        want[i, :min(156, len(soft))] = soft[:156]
    for fmt, dx in ((0, torch.from_numpy(xq).cuda()), (1, torch.from_numpy(xq).to(torch.float16).cuda())):
        soft = torch.full((B, 157), -1.0, device=dev)
        t1._chk(L.trxsig_equalize_taps_batch_fmt(t1.h, dx.data_ptr(), fmt, doff.data_ptr(), dlen.data_ptr(), B, damp.data_ptr(),
                                                 dtoa.data_ptr(), en.data_ptr(), dw.data_ptr(), db.data_ptr(), soft.data_ptr(), None,
                                                 156, 157), "equalize_taps_fmt")
        torch.cuda.synchronize()
        got = soft.cpu().numpy()
        for i in range(B):
            n = min(156, int(lens[i]))
            assert np.array_equal(got[i, :n], want[i, :n]), (fmt, i, int(lens[i]), float(toa[i]), int(kinds[i]))
