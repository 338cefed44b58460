"""GPU tests of mobile-side acquisition (include/trxsig_l1acq.h) against tests/l1_acq_model.py, at sps 1 and 4.

  stage 1   against the float64 metric within tol = 8 (L + 8) 2^-24 (7.2e-5 at sps 1, 2.7e-4 at sps 4): the frequency burst at
            k = 0, at the last k, across a segment and a tile boundary, quiet beside slots 40 dB up (the case that tells the
            summation schemes apart), a stream holding a NaN and an infinity, N < L + sps, more streams than one row of
            workgroups
  stage 2   exact: the model fed with the window and the shift the library reported; trxsig_l1acq_detect_sch_batch on
            caller-chosen windows (no shift, too short, the peak at the edge, the bogus and numRms paths, bad windows);
            trxsig_fec_sch_decode_batch against the l1msrx model
  truth     16 seeded streams per sps at 20 dB, |f| <= 0.1 cycle / symbol: state 15, BSIC, FN, the SCH start within 0.25 sample,
            the offset within 2e-3 cycle / symbol; the negative families
  closed loop   the reported frame grid -> the SCH slots of the following multiframe -> detect_sch -> L1MsRx.decode: all sync
Exact ties, every angle, sps 2 and a reused object: tests/test_gpu_acq_family.py on the family of tests/acq_family.py."""
import numpy as np
import pytest

import _pkg
import fec_stream_model as fsm
import fectxbind
import l1_acq_model as am
import l1_msrx_model as lrm
import oraclebind

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def tx():
    return fectxbind.FecTxOracle()


class Rig:
    def __init__(self, pkg, sps):
        self.pkg, self.sps = pkg, sps
        self.ctx = pkg.TrxSig(sps, 0)
        self.ctx.use_torch_stream()
        self.det = am.SchDetector(oraclebind.Oracle(sps))
        self.o = self.det.o

    def search(self, streams, fcch_thresh=0.5, sch_thresh=8.0, acq=None):
        """streams: equally long complex64 arrays -> L1Acq.collect()"""
        import torch
        N = len(streams[0])
        assert all(len(x) == N for x in streams)
        stride = N + 3                                         # a stride that is not the length
        buf = np.zeros((len(streams), stride), np.complex64)
        for i, x in enumerate(streams):
            buf[i, :N] = x
        d = torch.from_numpy(buf.view(np.float32)).cuda()
        own = acq is None
        acq = acq or self.pkg.L1Acq(self.ctx, len(streams), N)
        acq.search(d, stride, N, len(streams), fcch_thresh, sch_thresh)
        g = acq.collect()
        if own:
            acq.destroy()
        return g


@pytest.fixture(scope="module", params=[1, 4])
def rig(request, pkg):
    return Rig(pkg, request.param)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_stage1(g, i, x, sps, what):
    """the issue's stage-1 conditions for stream i of a search against the float64 metric of x"""
    L, tol = am.fcch_len(sps), am.fcch_tol(sps)
    C64, E64, m64 = am.fcch_metric64(x, sps)
    k = int(g["fcch_k"][i])
    assert 0 <= k < len(m64), (what, k)
    m, C = float(g["fcch_metric"][i]), complex(g["fcch_c"][i])
    print("%s: k %d (float64 argmax %d), m %.6f, m64[k] %.6f, max m64 %.6f, |dm| %.2e (tol %.2e), |dC| / E %.2e"
          % (what, k, int(np.argmax(m64)), m, m64[k], m64.max(), abs(m - m64[k]), tol, abs(C - C64[k]) / max(E64[k], 1e-30)))
    assert m64[k] >= m64.max() - tol, what
    assert abs(m - m64[k]) <= tol, what
    if m64.max() == 0:
        assert k == 0 and m == 0, what                         # every window scores 0: the answer is the first one
    arg = float(g["arg"][i])
    if np.isfinite(C):                                         # C, E, the angle and the shift, whatever the window scores
        assert abs(C - C64[k]) <= 2 * (L + 8) * 2.0 ** -24 * E64[k], what
        assert abs(float(g["fcch_e"][i]) - E64[k]) <= 2 * (L + 8) * 2.0 ** -24 * E64[k], what
        assert abs(arg - np.arctan2(float(g["fcch_c"][i].imag), float(g["fcch_c"][i].real))) <= 2e-6, what
    else:                                                      # only a window that holds a NaN or an infinity: score 0, angle 0
        assert not np.isfinite(x[k:k + L + sps]).all() and m == 0 and arg == 0, what
    assert g["omega"][i] == np.float32(-g["arg"][i] / np.float32(sps)), what
    return k, m64


def check_stage2(rig, tx, g, i, x, what, sch_thresh=8.0):
    """stream i of a search against the model fed with the library's window and shift: everything equal"""
    r = am.search_model(rig.det, tx, x, 0.5, sch_thresh, k=int(g["fcch_k"][i]), omega=g["omega"][i])
    assert int(g["state"][i]) == r["state"], (what, int(g["state"][i]), r["state"])
    if r["state"] & 1:
        assert int(g["sch_w0"][i]) == r["w0"], what
    if r["state"] & 2:
        s = r["sch"]
        assert g["sch_ptm"][i] == s["ptm"] and g["sch_amp"][i] == s["amp"] and g["sch_toa"][i] == s["toa"], \
            (what, g["sch_ptm"][i], s["ptm"], g["sch_amp"][i], s["amp"], g["sch_toa"][i], s["toa"])
        assert np.array_equal(g["soft"][i, :148], s["soft"]), (what, np.abs(g["soft"][i, :148] - s["soft"]).max())
        assert (bool(g["ok"][i]), int(g["bsic"][i]), int(g["rfn"][i])) == (r["ok"], r["bsic"], r["rfn"]), what
    else:
        assert not g["soft"][i].any() and g["sch_ptm"][i] == 0 and g["sch_amp"][i] == 0, what
    return r


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------
def tone_of(frame, sps):
    """where the L-window of the frequency burst of stream frame `frame` starts in the clean stream"""
    return frame * 1250 * sps + 3 * sps


def make_stage1(rig, tx, N, seed, frame, cut, loud=1.0, snr=30.0, f=0.03):
    """N samples with ONE frequency burst, in stream frame `frame`, cut in at `cut`"""
    rng = np.random.default_rng(seed)
    clean, _ = am.build_stream(rig.o, tx, rng, 10 - frame % 10 if frame % 10 else 10, 13, 7, keep={frame, frame + 1}, loud=loud)
    x = am.impair(clean, rng, rig.sps, cut, 0, f, 1.0, snr)
    assert len(x) >= N
    return x[:N]


def stage1_streams(rig, tx):
    """five streams of one length N (no multiple of the segment or of the tile), each with ONE frequency burst (fn0 = 10: frame 0
    and every tenth carry FCCH; keep picks one)"""
    sps, o = rig.sps, rig.o
    N = 15146 * sps - 37
    L, W = am.fcch_len(sps), 1136
    assert N % L and N % W
    out = []

    make = lambda *a, **kw: make_stage1(rig, tx, N, *a, **kw)
    tone = lambda frame: tone_of(frame, sps)
    out.append(("k = 0", make(1, 0, tone(0)), 0))
    out.append(("last k", make(2, 12, 37), N - sps - L))        # tone(12) - 37 = N - sps - L
    assert tone(12) - 37 == N - sps - L
    kt = (tone(5) // W) * W - L // 2                            # half the window in the last segment of a tile, half in the next
    out.append(("tile boundary", make(3, 5, tone(5) - kt), kt))
    out.append(("40 dB neighbours", make(4, 3, 11, loud=100.0, snr=None, f=-0.07), tone(3) - 11))
    x = make(5, 4, 23)
    x[1000] = np.nan
    x[tone(4) - 23 + L + 3000] = np.inf
    out.append(("NaN and infinity", x, tone(4) - 23))
    return N, out


def test_stage1_against_float64(rig, tx):
    sps = rig.sps
    N, cases = stage1_streams(rig, tx)
    g = rig.search([x for _, x, _ in cases])
    alone = rig.search([x for _, x, _ in cases[:4]])           # the same streams without the poisoned one
    for i, (what, x, where) in enumerate(cases):
        k, m64 = check_stage1(g, i, x, sps, "sps %d %s" % (sps, what))
        assert abs(k - where) <= 4 * sps and g["fcch_metric"][i] > 0.9 and g["state"][i] & 1, (what, k, where)
    for key in ("fcch_k", "fcch_metric", "fcch_c", "fcch_e", "arg", "omega", "state", "soft"):
        assert np.array_equal(g[key][:4], alone[key]), key     # a NaN in one stream leaves the others untouched
    # a frequency burst that holds a NaN cannot win: its windows score 0
    what, x, where = cases[2]
    y = x.copy()
    y[where + 71 * sps] = np.nan                               # the middle of the tone: no window beside it holds half of it
    ks = (tone_of(7, sps) // 1136) * 1136 + am.fcch_len(sps) // 2   # half in a tile's first segment, half in its second
    seg = make_stage1(rig, tx, N, 6, 7, tone_of(7, sps) - ks)
    gp = rig.search([y, x, seg])
    k, m64 = check_stage1(gp, 0, y, sps, "sps %d poisoned burst" % sps)
    assert abs(k - where) >= am.fcch_len(sps) // 2 and m64[where] == 0 and gp["fcch_metric"][0] < 0.5 and gp["state"][0] == 0
    check_stage1(gp, 1, x, sps, "sps %d beside it" % sps)
    k, _ = check_stage1(gp, 2, seg, sps, "sps %d segment boundary inside a tile" % sps)
    assert abs(k - ks) <= 4 * sps and (k % 1136) // am.fcch_len(sps) == 0 and gp["fcch_metric"][2] > 0.9, (k, ks)


def test_no_window_and_many_streams(rig, tx):
    sps = rig.sps
    L = am.fcch_len(sps)
    rng = np.random.default_rng(11)
    short = [(rng.standard_normal(L + sps - 1) + 1j * rng.standard_normal(L + sps - 1)).astype(np.complex64) for _ in range(3)]
    g = rig.search(short)
    assert (g["fcch_k"] == -1).all() and not g["state"].any() and not g["fcch_metric"].any() and not g["soft"].any()
    one = rig.search([x[:L + sps] for x in [np.concatenate([s, s[:1]]) for s in short]])      # exactly one window
    assert (one["fcch_k"] == 0).all()
    # every window scores 0: silence, and a stream with a NaN in every window -- k = 0, and C, E, the angle as the header says
    noise = (rng.standard_normal(3 * L) + 1j * rng.standard_normal(3 * L)).astype(np.complex64)
    poisoned = noise.copy()
    poisoned[L // 2::L // 2] = np.nan
    z = rig.search([np.zeros(3 * L, np.complex64), poisoned, noise])
    for i, x in enumerate((np.zeros(3 * L, np.complex64), poisoned, noise)):
        check_stage1(z, i, x, sps, "sps %d zero-metric %d" % (sps, i))
    assert (z["fcch_k"][:2] == 0).all() and not z["fcch_metric"][:2].any() and not z["state"][:2].any()
    assert z["fcch_c"][0] == 0 and z["fcch_e"][0] == 0 and z["arg"][0] == 0 and not np.isfinite(z["fcch_c"][1])
    # 70 streams of two frames and two slots: more streams than a wave, a block or one row of the grid hold
    clean, _ = am.build_stream(rig.o, tx, rng, 9, 3, 3)        # FCCH in frame 1, SCH in frame 2
    N = len(clean) - 1250 * sps
    streams = [am.impair(clean, rng, sps, int(c), int(c) % 8, 0.1 * np.sin(c), 1.0, 25.0)[:N] for c in np.linspace(0, 1100 * sps, 70)]
    g = rig.search(streams)
    for i in range(0, 70, 3):
        check_stage1(g, i, streams[i], sps, "sps %d stream %d of 70" % (sps, i))
        check_stage2(rig, tx, g, i, streams[i], "stream %d of 70" % i)
    assert (g["state"] & 1).sum() >= 60


# ---- truth and stage 2 on the shared cases ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth(rig, tx):
    cases = am.truth_cases(rig.sps)
    built = [am.truth_stream(rig.o, tx, c) for c in cases]
    return cases, built, rig.search([x for x, _ in built])


def test_truth(rig, tx, truth):
    sps = rig.sps
    cases, built, g = truth
    assert len(cases) >= 16 and len({c["fn0"] for c in cases}) >= 8 and any(c["fn0"] > am.HYPER - 20 for c in cases)
    worst_t = worst_f = 0.0
    for i, (case, (x, sch)) in enumerate(zip(cases, built)):
        check_stage1(g, i, x, sps, "sps %d truth %d" % (sps, i))
        assert g["state"][i] == 15, (i, case, g["state"][i])
        at = int(g["sch_w0"][i]) + float(g["sch_toa"][i])
        fn, true = min(sch, key=lambda s: abs(s[1] - at))
        assert (int(g["bsic"][i]), int(g["rfn"][i])) == (case["bsic"], fn), (i, case)
        worst_t = max(worst_t, abs(at - true))
        worst_f = max(worst_f, abs(float(g["arg"][i]) / (2 * np.pi) - case["f"]))
    print("sps %d: worst timing error %.3f sample, worst frequency error %.2e cycle / symbol" % (sps, worst_t, worst_f))
    assert worst_t <= 0.25 and worst_f <= 2e-3


def test_stage2_exact_in_a_search(rig, tx, truth):
    cases, built, g = truth
    for i, (x, _) in enumerate(built):
        r = check_stage2(rig, tx, g, i, x, "truth %d" % i)
        assert r["state"] == 15


def test_negative_families(rig, tx):
    sps = rig.sps
    neg = am.negative_streams(rig.o, tx, sps)
    for name, x in neg:
        g = rig.search([x])
        check_stage1(g, 0, x, sps, "sps %d %s" % (sps, name))
        check_stage2(rig, tx, g, 0, x, name)
        st = int(g["state"][0])
        if name == "no_fcch":
            assert st == 0 and g["fcch_metric"][0] < 0.5, (name, st, g["fcch_metric"][0])
        elif name == "no_sch":
            assert st == 3 and g["sch_ptm"][0] <= 8.0, (name, st, g["sch_ptm"][0])
        else:
            assert st == 1, (name, st)


# ---- stage 2 on caller-chosen windows --------------------------------------------------------------------------------------
def test_detect_sch_batch_exact(rig, tx):
    import torch
    sps, pkg = rig.sps, rig.pkg
    rng = np.random.default_rng(21)
    clean, slots = am.build_stream(rig.o, tx, rng, 10, 2, 33, extra_slots=2)
    f = 0.04
    x = am.impair(clean, rng, sps, 0, 3, f, 0.7 + 0.2j, 20.0)
    x0 = am.impair(clean, rng, sps, 0, 5, 0.0, 1.1j, 20.0)     # no offset: the window that is not shifted
    X = np.concatenate([x, x0])
    s = am.first(slots, "sch")[1]
    om = np.float32(-2 * np.pi * f / sps)
    B0 = len(x)
    wins = [(s - 12 * sps, 172 * sps, om), (B0 + s - 12 * sps, 172 * sps, None), (s - 12 * sps, 140 * sps, om),   # plain, unshifted, too short
            (s + 74 * sps, 100 * sps, om), (s - 98 * sps, 172 * sps, om),                        # half the sequence at either edge
            (s + 40 * sps, 2 * sps, om), (s, 1, om), (s - 3, 3 + 150 * sps + 1, om),             # numRms < 2; no whole symbols at the end
            (s - 100 * sps, 256 * sps, om), (s - 7 * sps - 1, 157 * sps, om), (s + 1, 148 * sps, om),
            (-1, 172 * sps, om), (s, 0, om), (s, 256 * sps + 1, om), (s + 300 * sps, 172 * sps, om)]   # bad windows; no SCH
    for shifted in (True, False):
        use = [w for w in wins if (w[2] is not None) == shifted]
        B = len(use)
        off, ln = np.array([w[0] for w in use], np.int32), np.array([w[1] for w in use], np.int32)
        flags, amp, toa, ptm = (torch.full((B,), 77, dtype=torch.uint8).cuda(), torch.ones(B, 2).cuda(), torch.ones(B).cuda(),
                                torch.ones(B).cuda())
        soft, hard = torch.ones(B, 150).cuda(), torch.ones(B, 150, dtype=torch.uint8).cuda()
        acq = pkg.L1Acq(rig.ctx, 1, 1000)                      # the workspace grows past max_streams on demand
        acq.detect_sch(dev(X.view(np.float32)), dev(off), dev(ln), flags, amp, toa, soft,
                       omega=dev(np.array([w[2] for w in use], np.float32)) if shifted else None, ptm=ptm, hard=hard)
        rig.ctx.synchronize()
        fl, a, t, p = flags.cpu().numpy(), amp.cpu().numpy().view(np.complex64).ravel(), toa.cpu().numpy(), ptm.cpu().numpy()
        sf, hd = soft.cpu().numpy(), hard.cpu().numpy()
        seen = set()
        for b, (o_, n_, w_) in enumerate(use):
            m = rig.det.detect(X[o_:o_ + n_], w_) if o_ >= 0 else dict(flags=128, amp=0, toa=0, ptm=0, soft=np.zeros(148, np.float32))
            what = "sps %d window %d (%d, %d)" % (sps, b, o_, n_)
            assert fl[b] == m["flags"], (what, fl[b], m["flags"])
            assert a[b] == m["amp"] and t[b] == m["toa"] and p[b] == m["ptm"], (what, a[b], m["amp"], t[b], m["toa"], p[b], m["ptm"])
            assert np.array_equal(sf[b, :148], m["soft"]) and np.array_equal(hd[b, :148], (m["soft"] > 0.5).astype(np.uint8)), what
            assert (sf[b, 148:] == 1).all() and (hd[b, 148:] == 1).all()           # nothing past 148 values is touched
            seen.add((int(fl[b]), bool(p[b] > 0)))
        acq.destroy()
        if shifted:
            assert fl[0] == 2 and fl[6] == 2 and fl[7] == 2 and fl[8] == 2, fl
            assert not fl[1:6].any() and fl[9] == 0 and p[4] == 0 and p[5] == 0 and (fl[10:13] == 128).all(), (fl, p)
            assert seen >= {(2, True), (0, True), (0, False), (128, False)}
        else:
            assert fl[0] == 2


def test_fec_sch_decode_batch(rig, tx):
    import torch
    rng = np.random.default_rng(31)
    fns = np.array([1, 51 * 5 + 11, 1326 * 2047 + 41, am.HYPER - 10, 51 * 100 + 31, 1326 * 5 + 51 * 7 + 21] * 3, np.uint32)
    bsic = rng.integers(0, 64, len(fns)).astype(np.uint8)
    bits = tx.sch_encode(fns, bsic)
    soft = fsm.soft_from_bits(rng, bits, 0.3)
    soft[6:12, rng.integers(3, 145, 30)] = 1 - soft[6:12, rng.integers(3, 145, 30)]    # corrupted rows
    soft[12:] = rng.random((6, 148)).astype(np.float32)                                 # noise rows
    soft = np.concatenate([soft, np.zeros((3, 148), np.float32)])                        # all-zero rows
    n, stride = len(soft), 151
    rows = np.ones((n, stride), np.float32)
    rows[:, :148] = soft
    ok, bs, rfn = torch.zeros(n, dtype=torch.uint8).cuda(), torch.zeros(n, dtype=torch.uint8).cuda(), torch.zeros(n, dtype=torch.int32).cuda()
    rig.ctx.fec_sch_decode(dev(rows), n, ok, bs, rfn)
    rig.ctx.synchronize()
    want = [lrm.sch_decode(tx, v) for v in soft]
    got = list(zip(ok.cpu().numpy().astype(bool), bs.cpu().numpy(), rfn.cpu().numpy()))
    assert [(bool(a), int(b), int(c)) for a, b, c in got] == [(bool(a), int(b), int(c)) for a, b, c in want]
    assert [w[0] for w in want[:6]] == [True] * 6 and [(int(b), int(c)) for _, b, c in got[:6]] == list(zip(bsic[:6].tolist(), fns[:6].tolist()))
    assert not any(w[0] for w in want[-3:])


def test_bad_arguments_and_lifetime(rig):
    import ctypes as C
    pkg, ctx, L = rig.pkg, rig.ctx, rig.ctx.L
    before = L.trxsig_live_children(ctx.h)
    acq = pkg.L1Acq(ctx, 2, 1000)
    assert L.trxsig_live_children(ctx.h) == before + 1
    d = dev(np.zeros(2 * 2000, np.float32))
    out = pkg.L1AcqOut()
    call = lambda *a: L.trxsig_l1acq_search(acq.h, *a, C.byref(out))
    assert call(d.data_ptr(), 1000, 1000, 2, 0.5, 8.0) == 0
    assert call(None, 1000, 1000, 2, 0.5, 8.0) == EINVAL
    assert call(d.data_ptr(), 1000, 1000, 3, 0.5, 8.0) == EINVAL and call(d.data_ptr(), 1000, 1001, 2, 0.5, 8.0) == EINVAL
    assert call(d.data_ptr(), 999, 1000, 2, 0.5, 8.0) == EINVAL and call(d.data_ptr(), 1000, 0, 2, 0.5, 8.0) == EINVAL
    assert call(d.data_ptr(), 1000, 1000, 0, 0.5, 8.0) == EINVAL
    assert L.trxsig_l1acq_search(acq.h, d.data_ptr(), 1000, 1000, 2, 0.5, 8.0, None) == EINVAL
    assert L.trxsig_l1acq_detect_sch_batch(acq.h, d.data_ptr(), None, None, 1, None, 8.0, None, None, None, None, None, None, 148) == EINVAL
    assert L.trxsig_l1acq_detect_sch_batch(acq.h, None, None, None, 0, None, 8.0, None, None, None, None, None, None, 148) == 0
    for bad in ((0, 1000), (1, 0), (70000, 10), (4, 2 ** 30)):
        h = C.c_void_p()
        assert L.trxsig_l1acq_create(C.byref(h), ctx.h, *bad) == EINVAL and not h.value
    seq, gain, toa = acq.sequence()
    assert np.array_equal(seq, rig.det.seq) and gain == rig.det.gain and toa == rig.det.toa
    ctx.synchronize()
    acq.destroy()
    assert L.trxsig_live_children(ctx.h) == before


def test_exact_in_tolerance_mode(rig, tx, truth):
    cases, built, g = truth
    rig.ctx.set_soft_mode(rig.pkg.SOFT_TOLERANCE)
    try:
        g2 = rig.search([x for x, _ in built[:3]])
    finally:
        rig.ctx.set_soft_mode(rig.pkg.SOFT_EXACT)
    for key in g:
        assert np.array_equal(g2[key], g[key][:3]), key


# ---- closed loop -----------------------------------------------------------------------------------------------------------
def test_closed_loop_to_l1msrx(pkg, tx):
    """search -> the frame grid -> the SCH slots of the following multiframe -> detect_sch -> L1MsRx.decode: every entry syncs"""
    import torch
    sps, bsic, fn0 = 4, 45, 51 * 26 * 17 + 40
    rig = Rig(pkg, sps)
    rng = np.random.default_rng(41)
    clean, slots = am.build_stream(rig.o, tx, rng, fn0, 66, bsic)
    x = am.impair(clean, rng, sps, 1777, 5, 0.06, 0.5 - 0.4j, 20.0)
    n_search = 12 * 1250 * sps + 313 * sps
    buf = dev(x.view(np.float32))
    acq = pkg.L1Acq(rig.ctx, 1, len(x))
    acq.search(buf, len(x), n_search, 1)
    g = acq.collect()
    assert g["state"][0] == 15 and g["bsic"][0] == bsic
    whole = pkg.L1Acq(rig.ctx, 1, len(x))                      # the whole stream: more tiles than a wave of the second launch
    whole.search(buf, len(x), len(x), 1)
    gw = whole.collect()
    assert gw["state"][0] == 15 and gw["bsic"][0] == bsic and gw["fcch_metric"][0] >= g["fcch_metric"][0]
    whole.destroy()
    rfn, origin = int(g["rfn"][0]), int(g["sch_w0"][0]) + float(g["sch_toa"][0])   # bit 0 of TN 0 of frame rfn
    fn_a, F = (rfn + 1) % am.HYPER, 51
    frames = [d for d in range(F) if (fn_a + d) % am.HYPER % 51 in am.SCH_T3]
    assert len(frames) == 5
    off = np.array([int(round(origin + (d + 1) * 1250 * sps)) - 12 * sps for d in frames], np.int32)
    assert off[-1] + 172 * sps <= len(x)
    B = len(off)
    flags, amp, toa, soft = torch.zeros(B, dtype=torch.uint8).cuda(), torch.zeros(B, 2).cuda(), torch.zeros(B).cuda(), torch.zeros(B, 148).cuda()
    acq.detect_sch(buf, dev(off), dev(np.full(B, 172 * sps, np.int32)), flags, amp, toa, soft,
                   omega=dev(np.full(B, g["omega"][0], np.float32)))
    rig.ctx.synchronize()
    assert (flags.cpu().numpy() == pkg.F_DETECT).all()
    assert np.abs(toa.cpu().numpy() - 12 * sps).max() <= 1.0   # the grid holds over the multiframe
    plan = np.array([[5, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
    row = np.full((8 * F, 1), -1, np.int32)
    row[[8 * d for d in frames], 0] = np.arange(B)
    drow = dev(row)
    res = pkg.TrxGroupResult(n_slots=8 * F, n_arfcn=1, n_rows=B, d_row=drow.data_ptr(), d_valid=flags.data_ptr(), d_flags=None,
                             d_amp=amp.data_ptr(), d_toa=toa.data_ptr(), d_avgpwr=None, d_threshold=None, d_soft=soft.data_ptr(),
                             soft_stride=148)
    rx = pkg.L1MsRx(rig.ctx, plan, bsic, 900)
    rx.decode(res, fn_a, True)
    sch = rx.collect(state=False)["sch"]
    assert len(sch["sync"]) == 5 and sch["present"].all() and sch["sync"].all(), sch
    assert [int(v) for v in sch["rfn"]] == [(fn_a + d) % am.HYPER for d in frames]
    rx.destroy(); acq.destroy()
