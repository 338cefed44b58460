"""GPU parity of the TOLERANCE-mode demodulator (trxsig_set_soft_mode(ctx, TRXSIG_SOFT_TOLERANCE); csrc/trxsig_demod.h,
fused_demod_tol) against the oracle and the golden vectors captured from the real reference:
  * flags, amplitude, TOA, avgPwr: value-exact (IEEE ==), as in the exact mode;
  * hard bits: identical, every burst, every bit;
  * soft bits: the parity contract, |soft - reference soft| <= 1e-6 or <= 1e-4 |reference soft|, for every value; the
    guaranteed bound 9.2e-6 ZMAX = 3.7e-5 on the [0, 1] scale as a second assertion; the error actually measured is reported
    and held under 2e-6;
  * bit for bit against the correctly rounded CPU restatement of the fast form (oracle/tol_oracle.c): a burst it takes equals
    its soft bits (IEEE ==), a burst it hands over equals the exact mode's -- on random batches, on bursts built to straddle
    ZMAX, the slicer's guard and the wave-wide maximum, and on the adversarial family of tests/tol_family.py;
  * a burst the fast form must not take (NaN / infinity anywhere, max|x| * |1/amp| > ZMAX, a TOA off the 1/512 grid, a soft
    symbol within the guard band of the slicer's 0.5) equals the exact mode bit pattern for bit pattern;
  * every kernel that runs the fast form: k_demod (path 0, also beside the detector), k_normal_quad / k_normal_chain (paths 3-5;
    k_normal_fused, paths 1-2, stays exact), k_demod_rx (the group's front end); and the UDP wire bytes.
The exact mode stays the default and is what every other test file grades."""
import numpy as np
import pytest

import _pkg
import oraclebind
import synth
import tol_family as tf
from util import GpuBatch, assert_veq

pytestmark = pytest.mark.gpu

BOUND = tf.GUARANTEE * tf.ZMAX      # 3.7e-5, guaranteed; the kernel hands over anything it cannot guarantee
MEASURED = 2e-6         # what the arithmetic actually does on these inputs (a few 2^-24 * Z)


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = {s: pkg.TrxSig(s, 0) for s in (1, 2, 4)}
    for v in c.values():
        v.use_torch_stream()
        v.set_soft_mode(pkg.SOFT_TOLERANCE)
        assert v.soft_mode() == pkg.SOFT_TOLERANCE
    return c


def grade(soft, ref, what):
    """soft bits of detected bursts against the reference's by the parity contract (and the guaranteed bound); returns (max abs
    error, fraction of values that are not identical)."""
    soft = np.asarray(soft, np.float64); ref = np.asarray(ref, np.float64)
    assert not np.isnan(soft).any() and not np.isnan(ref).any(), what
    err = np.abs(soft - ref)
    ratio = tf.contract_ratio(soft, ref)
    assert ratio.max(initial=0.0) <= 1.0, (what, ratio.max(), ref.ravel()[ratio.argmax()], err.ravel()[ratio.argmax()])
    assert err.max(initial=0.0) <= BOUND, (what, err.max())
    return float(err.max(initial=0.0)), float((err > 0).mean()) if err.size else 0.0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def restated(sps, x, off, length, amp, toa, nsoft=148, device_off=None):
    """The CPU restatement's verdict and soft bits for k_demod.  An odd sample offset in the device's batch (device_off, default
    off) or an odd length takes k_demod's other path: exact."""
    pkg = _pkg.load()
    T = pkg.build_tables_host(sps).view(pkg.tables_dtype())[0]
    verdict, soft = oraclebind.demod_tol(T, x, off, length, amp, toa, tf.ZMAX, nsoft=nsoft)
    odd = ((np.asarray(off if device_off is None else device_off) | np.asarray(length)) & 1) == 1
    verdict[odd] = oraclebind.TOL_NOT_DEMODULATED
    return verdict, soft


def assert_matches_restatement(got, exact, verdict, soft_c, what):
    """got: the kernel's tolerance soft bits [B, nsoft]; exact: the exact mode's (= the oracle's) for the same bursts."""
    taken = verdict == oraclebind.TOL_TAKEN
    for b in np.flatnonzero(taken):
        assert np.array_equal(_bits(got[b]), _bits(soft_c[b])), "%s: burst %d is the fast form's, bit for bit" % (what, b)
    for b in np.flatnonzero(~taken):
        assert np.array_equal(_bits(got[b]), _bits(exact[b])), "%s: burst %d is handed over: the exact mode's" % (what, b)
    return int(taken.sum())


@pytest.mark.parametrize("name", ["normal_sps4.npz", "normal_sps1.npz"])
def test_golden_normal_tolerance(pkg, ctx, golden, name):
    g = golden(name)
    sps = int(g["sps"]); t = ctx[sps]
    worst = 0.0
    for tsc in range(8):
        sel = np.flatnonzero(g["tsc"] == tsc)
        gb = GpuBatch(g["x"], g["off"][sel], g["len"][sel], nsoft=148, stride=160)
        t.detect_demod_normal(gb.x, gb.off, gb.len, tsc, gb.flags, gb.amp, gb.toa, gb.soft, avgpwr=gb.pwr,
                              hard=gb.hard, detect_thresh=3.0, energy_thresh=-1.0, nsoft=148, soft_stride=160)
        r = gb.results()
        det = (r["flags"] & pkg.F_DETECT) != 0
        assert_veq(det, g["ok"][sel].astype(bool), "detect flags tsc %d" % tsc)
        assert_veq(r["amp"], g["amp"][sel], "amp"); assert_veq(r["toa"], g["toa"][sel], "toa")
        assert_veq(r["pwr"], g["energy_pwr"][sel], "energyDetect avgPwr")
        for j, i in enumerate(sel):
            if det[j]:
                assert_veq(r["hard"][j, :148], (g["soft"][i, :148] > 0.5).astype(np.uint8), "hard %d" % i)
                e, _ = grade(r["soft"][j, :148], g["soft"][i, :148], "soft %d" % i)
                worst = max(worst, e)
            else:
                assert not r["soft"][j, :148].any() and not r["hard"][j, :148].any()
            assert np.all(r["soft"][j, 148:] == -1.0)          # nothing written past nsoft
    assert worst <= MEASURED, worst


@pytest.mark.parametrize("sps,B,sigmas", [(4, 4096, None), (4, 4096, (0.0, 0.1, 0.5, 2.0)), (2, 1024, None), (1, 2048, None)])
def test_random_batch_vs_oracle_tolerance(pkg, ctx, sps, B, sigmas):
    o = oraclebind.Oracle(sps)
    for tsc in (0, 5):
        kw = {} if sigmas is None else {"sigmas": sigmas}
        x, off, length, meta = synth.normal_batch(sps, B, tsc, seed=1234 + tsc + 10 * sps, **kw)
        gb = GpuBatch(x, off, length, nsoft=148, stride=157)
        ctx[sps].detect_demod_normal(gb.x, gb.off, gb.len, tsc, gb.flags, gb.amp, gb.toa, gb.soft, avgpwr=gb.pwr,
                                     hard=gb.hard, energy_thresh=0.0, nsoft=148, soft_stride=157)
        r = gb.results()
        ok, amp, toa, soft = o.normal_batch(x, off, length, tsc, nsoft=148, nthreads=8)
        okb = ok.astype(bool)
        assert_veq((r["flags"] & pkg.F_DETECT) != 0, okb, "detect")
        assert_veq(r["amp"], amp, "amp"); assert_veq(r["toa"], toa, "toa")
        assert_veq(r["hard"][:, :148], (soft > 0.5).astype(np.uint8), "hard")
        assert not r["soft"][~okb][:, :148].any()
        e, frac = grade(r["soft"][okb][:, :148], soft[okb], "soft")
        assert e <= MEASURED * (4 if sigmas else 1), e         # (noisy bursts: a larger Z, the error scales with it)
        # the rearranged arithmetic did run (or this test grades the exact code against itself)
        assert frac > 0.02, frac
        # a burst whose max|x| * |1/amp| is above ZMAX must have been handed to the exact code
        for b in np.flatnonzero(okb):
            xs = x[off[b]:off[b] + length[b]]
            a = complex(amp[b]); inv = 1.0 / a
            Z = max(np.abs(xs.real).max(), np.abs(xs.imag).max()) * (abs(inv.real) + abs(inv.imag))
            if Z > tf.ZMAX * 1.0001:
                assert_veq(r["soft"][b, :148], soft[b], "burst %d (Z = %.1f) is the exact code's" % (b, Z))
        # every detected burst, bit for bit: the restatement's soft bits where it takes the fast form, the oracle's elsewhere
        sel = np.flatnonzero(okb)
        verdict, soft_c = restated(sps, x, off[sel], length[sel], amp[sel], toa[sel])
        n = assert_matches_restatement(r["soft"][sel, :148], soft[sel], verdict, soft_c, "random batch")
        assert n > 0.5 * len(sel) * (0.5 if sps == 1 else 1.0), (n, len(sel))


def test_nsoft_above_148_is_exact(pkg, ctx):
    sps, tsc, B = 4, 1, 512
    x, off, length, _ = synth.normal_batch(sps, B, tsc, seed=31)
    gb = GpuBatch(x, off, length, nsoft=156, stride=157)
    ctx[sps].detect_demod_normal(gb.x, gb.off, gb.len, tsc, gb.flags, gb.amp, gb.toa, gb.soft, hard=gb.hard, energy_thresh=0.0,
                                 nsoft=156, soft_stride=157)
    r = gb.results()
    ok, amp, toa, soft = oraclebind.Oracle(sps).normal_batch(x, off, length, tsc, nsoft=156, nthreads=8)
    assert_veq(r["soft"][:, :156], soft, "soft")


def test_hostile_bursts_equal_the_exact_mode(pkg):
    """trxsig_demodulate_batch with the caller's amplitude / TOA: every case the fast form must refuse, beside ordinary ones.
    The exact mode (graded against the oracle here as well, where the oracle's loop ends) is the reference for the bit patterns."""
    import torch
    sps, tsc = 4, 2
    dev = torch.device("cuda:0")
    te = pkg.TrxSig(sps, 0); te.use_torch_stream()
    tt = pkg.TrxSig(sps, 0); tt.use_torch_stream(); tt.set_soft_mode(pkg.SOFT_TOLERANCE)
    base_x, off, length, meta = synth.normal_batch(sps, 64, tsc, seed=77, sigmas=(0.0, 0.05))
    x = base_x.copy()
    amp = np.asarray(meta["amp"], np.complex64).copy()       # the channel the bursts were made with: soft symbols near +-1, Z about 1.5
    toa = np.zeros(64, np.float32)
    rng = np.random.default_rng(3)
    toa[:] = (rng.integers(-3 * 512, 6 * 512, 64) / 512.0).astype(np.float32)   # on the grid, |TOA| small
    cases = {}

    def burst(b):
        return slice(int(off[b]), int(off[b] + length[b]))
    cases["ordinary"] = list(range(0, 16))
    amp[16] = 0; cases["amp zero"] = [16]
    amp[17] = np.nan; cases["amp NaN"] = [17]
    amp[18] = complex(np.inf, 0); cases["amp inf"] = [18]
    toa[19] = np.float32(0.3); cases["TOA off the grid"] = [19]
    toa[20] = np.float32(np.nan); cases["TOA NaN"] = [20]
    toa[21] = np.float32(5000.0); cases["TOA out of range"] = [21]
    # (a TOA with a real fraction: with |frac| <= 0.01 delayVector does not filter and three samples in four are never read)
    x[burst(22)][100] = complex(np.nan, 0); toa[22] = np.float32(0.5); cases["a NaN sample"] = [22]
    x[burst(23)][200] = complex(0, np.inf); toa[23] = np.float32(1.25); cases["an infinite sample"] = [23]
    x[burst(24)] = 0; cases["all-zero samples (every soft symbol on the slicer's 0.5)"] = [24]
    x[burst(25)] *= np.float32(1e-20); amp[25] *= np.float32(1e-20); cases["tiny samples, tiny amplitude"] = [25]
    x[burst(26)] *= np.float32(1e20); amp[26] *= np.float32(1e20); cases["huge samples, huge amplitude"] = [26]
    amp[27] *= np.float32(0.01); cases["Z far above ZMAX"] = [27]
    toa[28] = np.float32(-2.0); cases["integer delay (no filter)"] = [28]
    toa[29] = np.float32(1.00390625); cases["fraction 0.996"] = [29]
    toa[30] = np.float32(14.5); cases["samples fall off the front of the staging area"] = [30]    # (an access burst's kind of delay)
    toa[35] = np.float32(200.25); cases["samples fall off the front of the staging area"].append(35)
    toa[31] = np.float32(-3.5); cases["the first soft symbol reads before the burst"] = [31]
    toa[32] = np.float32(-0.001953125); cases["fraction 1/512: below the filter threshold"] = [32]
    x[burst(33)] *= np.float32(1e-30); amp[33] *= np.float32(1e-30); cases["1/amp beyond 1e15"] = [33]
    x[burst(34)][::2] = 0; cases["every other sample zero"] = [34]
    cases["ordinary, second half"] = list(range(36, 64))

    def run(t):
        gb = GpuBatch(x, off, length, nsoft=148, stride=148)
        a = torch.from_numpy(amp.view(np.float32).reshape(-1, 2).copy()).to(dev)
        to = torch.from_numpy(toa.copy()).to(dev)
        t.demodulate(gb.x, gb.off, gb.len, a, to, gb.soft, hard=gb.hard, nsoft=148, soft_stride=148)
        r = gb.results()
        return r["soft"], r["hard"]

    se, he = run(te)
    st, ht = run(tt)
    assert np.array_equal(he, ht), "hard bits"
    must_be_exact = [k for k in cases if k not in ("ordinary", "ordinary, second half", "integer delay (no filter)", "fraction 0.996",
                                                   "the first soft symbol reads before the burst", "fraction 1/512: below the filter threshold",
                                                   "every other sample zero", "samples fall off the front of the staging area")]
    for k in must_be_exact:
        for b in cases[k]:
            assert np.array_equal(_bits(se[b]), _bits(st[b])), k
    for k in cases:
        for b in cases[k]:
            if k in must_be_exact:
                continue
            grade(st[b], se[b], k)
    # (and the ordinary bursts did take the fast form)
    diff = sum(int((_bits(se[b]) != _bits(st[b])).sum()) for b in cases["ordinary"])
    assert diff > 0
    # the exact mode against the oracle on the cases the oracle's loops finish on
    o = oraclebind.Oracle(sps)
    for k in ("ordinary", "integer delay (no filter)", "fraction 0.996", "the first soft symbol reads before the burst",
              "samples fall off the front of the staging area", "Z far above ZMAX", "every other sample zero"):
        for b in cases[k]:
            ref = o.demodulate(x[burst(b)], amp[b], toa[b])[:148]
            assert_veq(se[b][:len(ref)], ref, k)


def test_rach_tolerance(pkg):
    sps, B = 4, 1024
    t = pkg.TrxSig(sps, 0); t.use_torch_stream(); t.set_soft_mode(pkg.SOFT_TOLERANCE)
    x, off, length, meta = synth.rach_batch(sps, B, seed=55)
    gb = GpuBatch(x, off, length, nsoft=148, stride=148)
    t.detect_demod_rach(gb.x, gb.off, gb.len, gb.flags, gb.amp, gb.toa, gb.soft, hard=gb.hard, detect_thresh=5.0, energy_thresh=-1.0,
                        nsoft=148, soft_stride=148)
    r = gb.results()
    ok, amp, toa, soft = oraclebind.Oracle(sps).rach_batch(x, off, length, nthreads=8)
    okb = ok.astype(bool)
    assert_veq((r["flags"] & pkg.F_DETECT) != 0, okb, "detect")
    assert_veq(r["amp"], amp, "amp"); assert_veq(r["toa"], toa, "toa")
    assert_veq(r["hard"][:, :148], (soft[:, :148] > 0.5).astype(np.uint8), "hard")
    e, frac = grade(r["soft"][okb][:, :148], soft[okb][:, :148], "soft")
    assert e <= 4 * MEASURED and frac > 0.02, (e, frac)


def test_full_batch_sample_tolerance(pkg):
    """BASELINE config 2 at its full size in tolerance mode: a 1,024-burst sample against the oracle, the whole batch against
    the exact mode (hard bits, flags, amp, TOA identical; soft bits within the bound), deterministic to the bit."""
    import torch
    from openbts_ttsou_amd import synth as gsynth
    dev = torch.device("cuda:0")
    sps, tsc, B, NS = 4, 2, 65536, 148
    x, off, length, meta = gsynth.normal_batch_torch(sps, B, tsc, seed=77, device=dev)
    xf = torch.view_as_real(x).contiguous()
    t = pkg.TrxSig(sps, 0); t.use_torch_stream(); t.reserve(B)

    def run():
        r = dict(flags=torch.zeros(B, dtype=torch.uint8, device=dev), amp=torch.zeros(B, 2, device=dev), toa=torch.zeros(B, device=dev),
                 soft=torch.full((B, NS), -1.0, device=dev), hard=torch.zeros((B, NS), dtype=torch.uint8, device=dev))
        t.detect_demod_normal(xf, off, length, tsc, r["flags"], r["amp"], r["toa"], r["soft"], hard=r["hard"], detect_thresh=3.0,
                              energy_thresh=0.0, nsoft=NS, soft_stride=NS)
        torch.cuda.synchronize()
        return r
    exact = run()
    t.set_soft_mode(pkg.SOFT_TOLERANCE)
    tol = run()
    tol2 = run()
    for k in ("flags", "amp", "toa", "hard"):
        assert torch.equal(exact[k], tol[k]), k
    assert torch.equal(tol["soft"].view(torch.int32), tol2["soft"].view(torch.int32))
    d = (exact["soft"].double() - tol["soft"].double()).abs()
    assert float(d.max().item()) <= MEASURED, float(d.max().item())
    assert float((d > 0).float().mean().item()) > 0.02
    # the contract over the whole batch, against the exact mode (whose soft bits are the reference's: test_gpu_fullsize.py)
    allow = torch.clamp(tf.REL * exact["soft"].double().abs(), min=tf.FLOOR)
    worst = float((d / allow).max().item())
    print("65,536 bursts: worst err / allowance %.3f" % worst)
    assert worst <= 1.0, worst
    # the UDP wire bytes, (char) round(soft * 255) (trxsig_trx_encode_rx_datagram): at most one count apart, rarely, and
    # identical for a burst the fast form handed over
    det = ((exact["flags"] & pkg.F_DETECT) != 0).cpu().numpy()
    se, st = exact["soft"].cpu().numpy(), tol["soft"].cpu().numpy()
    host = pkg.TrxHost(sps, 0)
    try:
        bytes_e = np.stack([np.frombuffer(host.encode_rx_datagram(0, 0, 0, 0, se[b]), np.uint8) for b in range(B)])
        bytes_t = np.stack([np.frombuffer(host.encode_rx_datagram(0, 0, 0, 0, st[b]), np.uint8) for b in range(B)])
    finally:
        host.close()
    wd = np.abs(bytes_e[det].astype(np.int32) - bytes_t[det].astype(np.int32))
    assert wd.max() <= 1, wd.max()
    n_diff = int((wd != 0).sum())
    print("wire bytes: %d of %d differ" % (n_diff, wd[:, 8:156].size))
    assert n_diff <= 1e-4 * wd[:, 8:156].size, n_diff
    rng = np.random.default_rng(9)
    pick = torch.from_numpy(np.sort(rng.choice(B, 1024, replace=False))).to(dev)
    offs = off[pick].cpu().numpy().astype(np.int64); lens = length[pick].cpu().numpy().astype(np.int64)
    xs = np.concatenate([xf[o:o + n].cpu().numpy().view(np.complex64).ravel() for o, n in zip(offs, lens)])
    so = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    ok, amp, toa, soft = oraclebind.Oracle(sps).normal_batch(xs, so, lens.astype(np.int32), tsc, nsoft=NS, nthreads=8)
    okb = ok.astype(bool)
    assert_veq(((tol["flags"][pick] & pkg.F_DETECT) != 0).cpu().numpy(), okb, "detect")
    assert_veq(tol["amp"][pick].cpu().numpy().view(np.complex64).ravel(), amp, "amp")
    assert_veq(tol["toa"][pick].cpu().numpy(), toa, "toa")
    assert_veq(tol["hard"][pick].cpu().numpy(), (soft > 0.5).astype(np.uint8), "hard")
    e, _ = grade(tol["soft"][pick].cpu().numpy()[okb], soft[okb], "soft")
    assert e <= MEASURED, e
    # the sample bit for bit against the restatement; the wire bytes of the bursts it hands over are the exact mode's
    sel = np.flatnonzero(okb)
    verdict, soft_c = restated(sps, xs, so[sel], lens[sel].astype(np.int32), amp[sel], toa[sel], device_off=offs[sel])
    picked = pick.cpu().numpy()[sel]
    assert_matches_restatement(tol["soft"][pick].cpu().numpy()[sel], soft[sel], verdict, soft_c, "65,536-burst sample")
    handed = picked[verdict != oraclebind.TOL_TAKEN]
    assert np.array_equal(bytes_e[handed], bytes_t[handed])


def test_group_on_the_fused_front_end_tolerance(pkg):
    """The Transceiver group on the fused receive front end (config 4's default call: schedule with access-burst slots, per-ARFCN
    threshold state, k_demod_rx) in tolerance mode against itself in exact mode, three pushes: valid / RSSI / timing / thresholds
    identical, hard bits identical, soft bits within the bound."""
    import torch
    from openbts_ttsou_amd import synth as gsynth
    from openbts_ttsou_amd.frontend import RxFrontEnd
    sps, S, K, tsc, pushes = 4, 16, 25, 2, 3
    dev = torch.device("cuda:0")
    nb = (K * pushes * 585 // 156 + 4 + 3) // 4 * 4
    x, off, length, meta = gsynth.normal_batch_torch(sps, S * nb, tsc, seed=91, device=dev, sigmas=(0.02, 0.05))
    hi = x.reshape(-1)[: S * (x.numel() // S)].reshape(S, -1)
    t = torch.arange(K * pushes * 864, device=dev, dtype=torch.float64) * (65.0 * sps / 96.0)
    i0 = t.floor().long().clamp(max=hi.shape[1] - 2); fr = (t - i0).to(torch.float32)
    lo = hi[:, i0] * (1 - fr) + hi[:, i0 + 1] * fr
    lo = lo * (8000.0 / lo.abs().amax(dim=1, keepdim=True))
    iq = torch.stack([lo.imag, lo.real], dim=2).round().clamp(-32768, 32767).to(torch.int16).contiguous()
    lpf = gsynth.design_lpf(961, 65 * sps)
    outs = []
    for mode in (pkg.SOFT_EXACT, pkg.SOFT_TOLERANCE):
        ctx = pkg.TrxSig(sps, 0); ctx.use_torch_stream(); ctx.set_soft_mode(mode)
        g = pkg.TrxGroup(ctx, S, tsc_leg=pkg.TSCLEG_DEMOD, start=(0, 0))
        fe = RxFrontEnd(ctx, S, lpf, max_chunks=K)
        for a in range(S):
            g.control(a, "CMD SETTSC %d" % tsc)
            for tn in range(8):
                g.control(a, "CMD SETSLOT %d %d" % (tn, 5 if (tn == 0 and a % 4 == 0) else 1))
        got, slots = [], 0
        for p in range(pushes):
            ns, _ = g.pull_rxfe(fe, iq[:, p * K * 864:(p + 1) * K * 864], (slots // 8))
            got.append(g.collect()); slots += ns
        outs.append(got)
        fe.close(); g.close(); ctx.close()
    n_valid = 0
    worst = 0.0
    for a, b in zip(*outs):
        for key in ("valid", "rssi", "timing", "threshold"):
            assert np.array_equal(a[key], b[key], equal_nan=True), key
        v = a["valid"]
        n_valid += int(v.sum())
        assert np.array_equal(a["soft"][v] > 0.5, b["soft"][v] > 0.5)
        e, _ = grade(b["soft"][v], a["soft"][v], "k_demod_rx")       # by the contract, against the exact mode
        worst = max(worst, e)
        assert np.array_equal(a["soft"][~v], b["soft"][~v])
    assert n_valid > 500 and 0 < worst <= 4 * MEASURED, (n_valid, worst)


def _demod_both(pkg, sps, x, off, length, amp, toa):
    """trxsig_demodulate_batch with the caller's amp / TOA in both modes: (exact soft, tolerance soft, exact hard, tolerance hard)."""
    import torch
    dev = torch.device("cuda:0")
    out = []
    for mode in (pkg.SOFT_EXACT, pkg.SOFT_TOLERANCE):
        t = pkg.TrxSig(sps, 0); t.use_torch_stream(); t.set_soft_mode(mode)
        gb = GpuBatch(x, off, length, nsoft=148, stride=148)
        a = torch.from_numpy(np.ascontiguousarray(amp, np.complex64).view(np.float32).reshape(-1, 2).copy()).to(dev)
        to = torch.from_numpy(np.ascontiguousarray(toa, np.float32).copy()).to(dev)
        t.demodulate(gb.x, gb.off, gb.len, a, to, gb.soft, hard=gb.hard, nsoft=148, soft_stride=148)
        r = gb.results()
        t.close()
        out.append(r)
    return out[0]["soft"], out[1]["soft"], out[0]["hard"], out[1]["hard"]


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_adversarial_family_on_the_device(pkg, sps):
    """tests/tol_family.py's adversarial family (large partial sums cancelled into the low band) through k_demod: by the contract,
    and bit for bit against the restatement; the exact mode is the oracle's."""
    T = pkg.build_tables_host(sps).view(pkg.tables_dtype())[0]
    B = 1024 * 4 // sps
    x, off, length, amp, toa, steered = tf.adversarial_batch(T, sps, B, tf.ZMAX, seed=606 + sps)
    se, st, he, ht = _demod_both(pkg, sps, x, off, length, amp, toa)
    ref = oraclebind.Oracle(sps).demod_batch(x, off, length, amp, toa, nthreads=8)
    assert_veq(se, ref, "exact mode")
    assert np.array_equal(he, ht) and np.array_equal(he, (ref > 0.5).astype(np.uint8)), "hard bits"
    verdict, soft_c = restated(sps, x, off, length, amp, toa)
    n = assert_matches_restatement(st, se, verdict, soft_c, "adversarial sps %d" % sps)
    assert n > 0.8 * B, n
    grade(st, ref, "adversarial sps %d" % sps)
    assert (ref[steered & (verdict == oraclebind.TOL_TAKEN)[:, None]] < 0.0101).sum() > 5000


def _edge_batch(pkg, sps, rng):
    """Bursts at the edges the fast form decides on (labels alongside): Z at ZMAX (1 -+ 2^-20); one output's |re'| swept across
    the guard fma(Z, 2^-15, 2^-22); the burst's largest sample alone in one lane of each quarter of the wave."""
    T = pkg.build_tables_host(sps).view(pkg.tables_dtype())[0]
    grid = np.asarray(T["sinc_grid"], np.float32); rev = np.asarray(T["rev"], np.complex64)
    x0, off0, len0, amp0, toa0, _ = tf.adversarial_batch(T, sps, 96, 2.0, seed=int(rng.integers(1 << 30)))
    v0, _ = oraclebind.demod_tol(T, x0, off0, len0, amp0, toa0, tf.ZMAX)
    keep = np.flatnonzero(v0 == oraclebind.TOL_TAKEN)[:48]              # (bases the fast form takes as they are)
    assert len(keep) == 48
    x0 = np.concatenate([x0[off0[b]:off0[b] + len0[b]] for b in keep])
    off0, len0, amp0, toa0 = off0[:48], len0[keep], amp0[keep], toa0[keep]
    N = int(len0[0])
    bursts, labels, amps, toas = [], [], [], []

    def add(xb, a, t, label):
        bursts.append(np.asarray(xb, np.complex64)); amps.append(np.complex64(a)); toas.append(np.float32(t)); labels.append(label)

    def z(xb, a):
        return float(tf.z_of(xb, [0], [len(xb)], [a])[0])
    base = [x0[off0[b]:off0[b] + N].copy() for b in range(48)]
    # (1) Z at ZMAX (1 -+ 2^-20): the samples scaled, Z checked on the side wanted
    for b in range(8):
        for side in (-1, 1):
            c = tf.ZMAX * (1 + side * 2.0 ** -20) / z(base[b], amp0[b])
            xb = (base[b] * np.float32(c)).astype(np.complex64)
            assert (z(xb, amp0[b]) > tf.ZMAX) == (side > 0)
            add(xb, amp0[b], toa0[b], "Z %s ZMAX" % ("above" if side > 0 else "below"))
    # (2) one output steered to |re| = guard (1 + d), d swept across 0 (re computed in float64; the kernel's re' lands within a few
    #     2^-24 of it): the restatement says which side each burst is on, the kernel must agree
    for b in range(8, 40):
        xb, a, t = base[b].copy(), amp0[b], toa0[b]
        k = int(np.floor(-t)); f = int(round((-t - k) * 512))
        tp = grid[f, :21].astype(np.float64)
        inv = complex(tf.inv_of(a))
        m = 70 + int(rng.integers(0, 8)); tt = sps * m - k
        w = complex(rev[sps * m]) * inv
        idx = tt + 10 - np.arange(21)
        d = (b - 24) * 2.0 ** -9
        sign = 1.0 if b % 2 else -1.0
        for _ in range(3):                                   # (the centre sample moves Z a little: settle the guard)
            guard = z(xb, a) * 2.0 ** -15 + 2.0 ** -22
            rest = (w * (xb[idx].astype(np.complex128) * tp).sum() - w * tp[10] * complex(xb[idx[10]])).real
            xb[idx[10]] = np.complex64((sign * guard * (1 + d) - rest) / (tp[10] * abs(w) ** 2) * np.conj(w))
        add(xb, a, t, "guard")
    # (3) the largest sample alone in lane L of each quarter (k_demod: lane L holds samples 2 (L + 64 i), 2 (L + 64 i) + 1), with Z
    #     just above ZMAX (must be handed over) and just below (taken)
    for q, lane in enumerate((5, 22, 41, 63)):
        for side in (-1, 1):
            b = 40 + 2 * q + (side > 0)
            xb, a = base[b].copy(), amp0[b]
            n = 2 * (lane + 64 * int(rng.integers(0, (N // 2 - lane - 1) // 64 + 1))) + int(rng.integers(0, 2))
            inv = tf.inv_of(a); inv1 = float(np.float32(abs(np.float32(inv.real)) + abs(np.float32(inv.imag))))
            xb[n] = np.complex64(complex(tf.ZMAX * (1 + side * 2.0 ** -18) / inv1, 0.1))
            assert (z(xb, a) > tf.ZMAX) == (side > 0) and abs(xb[n].real) == max(np.abs(xb.real).max(), np.abs(xb.imag).max())
            add(xb, a, toa0[b], "max in lane %d, Z %s" % (lane, "above" if side > 0 else "below"))
    off = np.arange(len(bursts), dtype=np.int32) * N
    return np.concatenate(bursts), off, np.full(len(bursts), N, np.int32), np.array(amps), np.array(toas), labels


@pytest.mark.parametrize("sps", [1, 4])
def test_edges_bit_for_bit(pkg, sps):
    x, off, length, amp, toa, labels = _edge_batch(pkg, sps, np.random.default_rng(31 + sps))
    se, st, he, ht = _demod_both(pkg, sps, x, off, length, amp, toa)
    ref = oraclebind.Oracle(sps).demod_batch(x, off, length, amp, toa, nthreads=8)
    assert_veq(se, ref, "exact mode")
    assert np.array_equal(he, ht), "hard bits"
    verdict, soft_c = restated(sps, x, off, length, amp, toa)
    for b, lab in enumerate(labels):
        if "above" in lab:
            assert verdict[b] == oraclebind.TOL_HANDED_OVER, lab
        elif lab == "Z below ZMAX":                                  # (a large lone sample may put an output in the guard band)
            assert verdict[b] == oraclebind.TOL_TAKEN, lab
    g = np.array([lab == "guard" for lab in labels])
    # the sweep crosses the guard: both verdicts occur
    assert (verdict[g] == oraclebind.TOL_TAKEN).any() and (verdict[g] == oraclebind.TOL_HANDED_OVER).any(), verdict[g]
    assert_matches_restatement(st, se, verdict, soft_c, "edges sps %d" % sps)
    grade(st, ref, "edges")


def _normal_fused_hostile(sps, tsc, seed):
    import test_gpu_normal_fused as nf
    return nf.hostile_batch(sps, tsc, seed)


@pytest.fixture(scope="module")
def tol_ctxs(pkg):
    """Tolerance-mode contexts on every normal-burst path: path 0 (k_demod after the detector; the product library), path 0 with
    the demodulator beside the detector, paths 1-5 (k_normal_fused, k_normal_quad, k_normal_chain; tuning library)."""
    c = {}
    for key in [0, "beside", 1, 2, 3, 4, 5]:
        for s in (1, 2, 4):
            t = pkg.TrxSig(s, 0, tuning=(key not in (0, "beside")))
            t.use_torch_stream()
            if key == "beside":
                t.set_tuning(demod_beside=1)
            elif key != 0:
                t.set_tuning(normal_path=key)
            t.set_soft_mode(pkg.SOFT_TOLERANCE)
            c[key, s] = t
    yield c
    for t in c.values():
        t.close()


def _run_normal(t, x, off, length, tsc, energy_thresh):
    gb = GpuBatch(x, off, length, nsoft=148, stride=148)
    t.detect_demod_normal(gb.x, gb.off, gb.len, tsc, gb.flags, gb.amp, gb.toa, gb.soft, avgpwr=gb.pwr, hard=gb.hard,
                          detect_thresh=3.0, energy_thresh=energy_thresh, nsoft=148, soft_stride=148)
    return gb.results()                                     # (a device-wide synchronize: the side stream's demodulator included)


@pytest.mark.parametrize("path", ["beside", 1, 2, 3, 4, 5])
@pytest.mark.parametrize("sps", [1, 2, 4])
def test_every_call_site_tolerance(pkg, tol_ctxs, sps, path):
    """The random batch and the hostile windows of test_gpu_normal_fused.py in tolerance mode: flags, amp, TOA and hard bits are
    the oracle's; soft bits graded by the contract and equal to path 0's tolerance output bit for bit (paths 3-5 and the side
    stream run fused_demod_tol too), path 0's equal to the restatement's.  A burst of odd offset or length, which k_demod and k_normal_chain
    send to the exact form and k_normal_quad does not, is either the restatement's fast form or the exact one.  Paths 1 and 2
    (k_normal_fused, one and two bursts per wave) have no tolerance form: their soft bits stay the oracle's."""
    o = oraclebind.Oracle(sps)
    batches = []
    for tsc in (0, 5):
        x, off, length, _ = synth.normal_batch(sps, {4: 2051, 2: 1025, 1: 2050}[sps], tsc, seed=4321 + tsc + 10 * sps)
        batches.append(("random tsc %d" % tsc, x, off, length, tsc, 0.0))
    for tsc in (2, 7):
        x, off, length = _normal_fused_hostile(sps, tsc, seed=99 + tsc)
        batches.append(("hostile tsc %d" % tsc, x, off, length, tsc, -1.0))
    n_diff = 0
    for what, x, off, length, tsc, ethr in batches:
        r = _run_normal(tol_ctxs[path, sps], x, off, length, tsc, ethr)
        r0 = _run_normal(tol_ctxs[0, sps], x, off, length, tsc, ethr)
        ok, amp, toa, soft = o.normal_batch(x, off, length, tsc, nsoft=148, nthreads=8)
        okb = ok.astype(bool)
        assert_veq((r["flags"] & pkg.F_DETECT) != 0, okb, "%s: detect" % what)
        assert_veq(r["amp"], amp, "%s: amp" % what); assert_veq(r["toa"], toa, "%s: toa" % what)
        assert_veq(r["hard"], (soft > 0.5).astype(np.uint8), "%s: hard" % what)
        if path in (1, 2):
            assert_veq(r["soft"], soft, "%s: k_normal_fused stays exact" % what)
            continue
        sel = np.flatnonzero(okb)
        verdict, soft_c = restated(sps, x, off[sel], length[sel], amp[sel], toa[sel])
        assert_matches_restatement(r0["soft"][sel], soft[sel], verdict, soft_c, "%s: path 0" % what)
        even = ((off | length) & 1) == 0
        assert_veq(r["soft"][even], r0["soft"][even], "%s: soft = path 0's tolerance output" % what)
        v_any, c_any = oraclebind.demod_tol(pkg.build_tables_host(sps).view(pkg.tables_dtype())[0], x, off[sel], length[sel],
                                            amp[sel], toa[sel], tf.ZMAX)
        for i, b in enumerate(sel):
            if not even[b]:
                assert (np.array_equal(_bits(r["soft"][b]), _bits(soft[b])) or
                        (v_any[i] == oraclebind.TOL_TAKEN and np.array_equal(_bits(r["soft"][b]), _bits(c_any[i])))), (what, b)
        assert not r["soft"][~okb].any()
        grade(r["soft"][okb], soft[okb], what)
        n_diff += int((_bits(r["soft"][okb]) != _bits(soft[okb])).sum())
    assert (n_diff > 0) == (path not in (1, 2)), n_diff              # (the fast form did run on this path, or not at all)
