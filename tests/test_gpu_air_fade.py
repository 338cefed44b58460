"""GPU tests of the fading-tap generator (include/trxsig_air.h, "Time-varying multipath") against tests/air_fade_model.py, at
sps 1 and 4, on 3 columns x 2 frames.

  profiles      "one": P = 1, S = 1, 1 tap, centre 0; "full": P = 12, S = 32 (396 pairs: six trips and 12 lanes of a seventh) with
                two line-of-sight paths (one of them nothing but line of sight), 32 taps, centre 4; "odd": P = 5, S = 6 (35 pairs:
                no multiple of 64), 5 taps, centre 0
  params        trxsig_air_fade_params equals the model word for word (Doppler 0, 1, 2^31 - 1 and a word with the top bit set
                among the links)
  taps          every component within the header's bound of the float64 model, with d_link NULL and with explicit links --
                ids below 0 and at n_links give taps that are all +0; the words behind the array untouched
  determinism   two runs bit-equal; F = 2 equals 1 + 1; a 1-column call equals that column of the 3-column call (column 0 by the
                defaults, column 2 through fade_columns and its links); an array that is not 16-byte aligned (8-byte stores)
                holds the words of an aligned one (16-byte stores)
  wrap          fn = 2715647 with F = 2 crosses the hyperframe's wrap as the model does, and equals the two calls either side
  through cells with D = 0 and one whole-sample path, trxsig_air_cells driven by the generated taps equals AirModel driven by the
                same taps word for word
  refusals      the argument rules that need a live object"""
import numpy as np
import pytest

import _pkg
import air_fade_model as fm
import air_model as am
import oraclebind

pytestmark = pytest.mark.gpu
EINVAL = -1
GUARD = np.float32(-777.25)
A, F = 3, 2
Q23 = 1 << 23

PROFILES = {
    "one": dict(delay_ns=[0], power=[1.0], n_sinusoids=1, n_taps=1, centre=0),
    "full": dict(delay_ns=[0, 100, 200, 400, 700, 1100, 1600, 2300, 3100, 3700, 4400, 5000],
                 power=[0.2, 0.15, 0.1, 0.1, 0.1, 0.08, 0.07, 0.06, 0.05, 0.04, 0.03, 0.02],
                 los_share=[0.7, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0.25], los_cos_q23=[Q23 // 2, 0, 0, -Q23, 0, 0, 0, 0, 0, 0, 0, Q23],
                 n_sinusoids=32, n_taps=32, centre=4),
    "odd": dict(delay_ns=[0, 300, 900, 2100, 3700], power=[0.4, 0.3, 0.15, 0.1, 0.05], n_sinusoids=6, n_taps=5, centre=0),
}


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_u32(a):
    return dev(np.ascontiguousarray(a, np.uint32).view(np.int32))


def words(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


class Rig:
    def __init__(self, pkg, sps):
        self.pkg, self.sps = pkg, sps
        self.ctx = pkg.TrxSig(sps, 0)
        self.ctx.use_torch_stream()
        self.air = pkg.Air(self.ctx)
        self._models = {}

    def model(self, name, col_khz=None):
        key = (name, None if col_khz is None else tuple(col_khz))
        if key not in self._models:
            self._models[key] = fm.FadeModel(self.sps, col_khz=col_khz, **PROFILES[name])
        return self._models[key]

    def profile(self, name, col_khz=None):
        self.air.fade_profile(**PROFILES[name])
        self.air.fade_columns([200 * a for a in range(A)] if col_khz is None else col_khz)

    def fade(self, fn, n_arfcn, n_frames, seed, dop, link=None, skew=0):
        """-> complex64 [n_arfcn][8 n_frames][n_taps]; skew: complex samples the array starts after a 16-byte boundary"""
        import torch
        n = n_arfcn * 8 * n_frames * self.air.fade_shape[2]
        buf = torch.full((2 * (n + skew) + 64,), float(GUARD), dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        self.air.fade(fn, n_arfcn, n_frames, seed, len(dop), dev_u32(dop), buf.data_ptr() + 8 * skew,
                      None if link is None else dev(np.asarray(link, np.int32)))
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert (h[:2 * skew] == GUARD).all() and (h[2 * (skew + n):] == GUARD).all(), "written outside the array"
        return h[2 * skew:2 * (skew + n)].view(np.complex64).reshape(n_arfcn, 8 * n_frames, -1).copy()


@pytest.fixture(scope="module", params=[1, 4])
def rig(request, pkg):
    return Rig(pkg, request.param)


def doppler(n_links, seed):
    d = np.random.default_rng(seed).integers(0, 1 << 31, n_links).astype(np.uint32)
    d[:4] = [0, 1, (1 << 31) - 1, 0x80000000 | 12345]
    return d


def explicit_links(n_links):
    """[A][8 F]: every cell its own choice, with ids below 0 and at n_links and beyond among them"""
    link = np.random.default_rng(3).integers(0, n_links, (A, 8 * F)).astype(np.int32)
    link[0, 0], link[1, 5], link[2, 15], link[0, 9], link[1, 1] = -1, n_links, n_links + 7, -(1 << 31), n_links - 1
    return link


def check_bound(tag, got, m, want, dead=None):
    """every component within the model's bound; -> the largest deviation as a share of the bound"""
    bound = m.bound()
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))          # [a][t][j]
    worst = err.max(axis=(0, 1))
    share = (worst[bound > 0] / bound[bound > 0]).max()         # (a tap that no path reaches has weight 0, bound 0 and error 0)
    print("%s: largest |device - float64 model| %.3e (bound %.3e there); worst share of the bound %.4f" %
          (tag, err.max(), bound[np.argmax(worst)], share))
    assert (err <= bound).all()
    if dead is not None:
        assert not words(got[dead]).any(), "a cell without a link is not +0"
        assert np.abs(got[~dead]).max() > 0
    return err.max(), share


@pytest.mark.parametrize("name", list(PROFILES))
def test_params_words(rig, name):
    import torch
    m = rig.model(name)
    L, seed = 29, 0xfeedc0de12345678
    dop = doppler(L, 1)
    rig.profile(name)
    n = L * m.P * (m.S + 1)
    phase = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    step = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    rig.air.fade_params(seed, L, dev_u32(dop), phase, step)
    torch.cuda.synchronize()
    phi, st = m.params(seed, L, dop)
    assert not phase[n:].any() and not step[n:].any()
    gp, gs = phase.cpu().numpy()[:n].view(np.uint32).reshape(phi.shape), step.cpu().numpy()[:n].reshape(st.shape)
    print("sps %d %s: %d phase words and %d steps differ of %d" % (rig.sps, name, (gp != phi).sum(), (gs != st).sum(), n))
    assert np.array_equal(gp, phi) and np.array_equal(gs, st)
    assert not gs[0].any() and gs[2].any()                      # D = 0 and D = 2^31 - 1


@pytest.mark.parametrize("name", list(PROFILES))
def test_taps_within_bound(rig, name):
    m = rig.model(name)
    fn, seed, L = 123456, 0x0123456789abcdef, 8 * A
    dop = doppler(L, 2)
    rig.profile(name)
    got = rig.fade(fn, A, F, seed, dop)
    check_bound("sps %d %s, default links" % (rig.sps, name), got, m, m.taps(fn, A, F, seed, L, dop))
    L = 11                                                      # fewer links than 8 A: the default links beyond are dead too
    dop = doppler(L, 3)
    link = explicit_links(L)
    got = rig.fade(fn, A, F, seed, dop, link)
    check_bound("sps %d %s, explicit links" % (rig.sps, name), got, m, m.taps(fn, A, F, seed, L, dop, link), (link < 0) | (link >= L))
    got = rig.fade(fn, A, F, seed, dop)
    t = np.arange(8 * F)
    check_bound("sps %d %s, default links, 11 of them" % (rig.sps, name), got, m, m.taps(fn, A, F, seed, L, dop),
                (8 * np.arange(A)[:, None] + t[None, :] % 8) >= L)


@pytest.mark.parametrize("name", list(PROFILES))
def test_determinism(rig, name):
    fn, seed, L = 2000000, 99, 8 * A
    dop = doppler(L, 4)
    link = explicit_links(L)
    rig.profile(name)
    whole = rig.fade(fn, A, F, seed, dop, link)
    assert np.array_equal(words(whole), words(rig.fade(fn, A, F, seed, dop, link)))
    assert np.array_equal(words(whole), words(rig.fade(fn, A, F, seed, dop, link, skew=1)))            # 8-byte stores
    parts = [rig.fade(fn + k, A, 1, seed, dop, link[:, 8 * k:8 * k + 8]) for k in range(F)]
    assert np.array_equal(words(whole), words(np.concatenate(parts, axis=1)))
    plain = rig.fade(fn, A, F, seed, dop)
    assert np.array_equal(words(plain[:1]), words(rig.fade(fn, 1, F, seed, dop)))
    rig.air.fade_columns([400])
    t = np.arange(8 * F)
    assert np.array_equal(words(plain[2:]), words(rig.fade(fn, 1, F, seed, dop, (16 + t % 8)[None, :])))
    for kw in (dict(seed=seed ^ 1), dict(seed=seed ^ (1 << 40)), dict(fn=fn + 1)):                     # other counters, other taps
        assert not np.array_equal(rig.fade(kw.get("fn", fn), 1, F, kw.get("seed", seed), dop), plain[:1])


def test_across_the_wrap(rig):
    name = "odd"
    m = rig.model(name)
    fn, seed, L = am.HYPER - 1, 5, 8 * A
    dop = doppler(L, 5)
    rig.profile(name)
    whole = rig.fade(fn, A, 2, seed, dop)
    check_bound("sps %d across the wrap" % rig.sps, whole, m, m.taps(fn, A, 2, seed, L, dop))
    parts = [rig.fade(fn, A, 1, seed, dop), rig.fade(0, A, 1, seed, dop)]
    assert np.array_equal(words(whole), words(np.concatenate(parts, axis=1)))
    # (the process jumps there: the second frame is frame 0's, not the frame after 2715647's in an unwrapped count)
    assert np.abs(whole[:, 8:] - m.taps(0, A, 1, seed, L, dop)).max() <= m.bound().max()


def test_cells_driven_by_the_generated_taps(rig):
    """D = 0 and one path a whole number of samples late (centre 2 of 5 taps): the taps are (0, 0, g, 0, 0) and stay put; the
    cell form run with them equals the oracle's convolve run with the same words"""
    import torch
    sps, T = rig.sps, 8 * F
    rig.air.fade_profile(delay_ns=[0], power=[0.8], n_sinusoids=9, n_taps=5, centre=2)
    rig.air.fade_columns([0, 200, 400])
    L = 8 * A
    taps_d = torch.zeros(A, T, 5, 2, dtype=torch.float32, device="cuda")
    rig.air.fade(77, A, F, 31, L, dev_u32(np.zeros(L, np.uint32)), taps_d)
    torch.cuda.synchronize()
    taps = taps_d.cpu().numpy().view(np.complex64).reshape(A, T, 5)
    assert np.count_nonzero(taps) == A * T and (taps[:, :, 2] != 0).all()
    assert np.array_equal(words(taps[:, :8]), words(taps[:, 8:]))                   # D = 0: frame 2 is frame 1
    assert len(np.unique(taps[0, :8, 2])) == 8                                      # eight links, eight gains
    x = am.random_cells(np.random.default_rng(9), A, T, sps)
    cell = 157 * sps
    buf = np.zeros((A, T, cell), np.complex64)
    for a in range(A):
        for t in range(T):
            buf[a, t, :len(x[a][t])] = x[a][t]
    d = dev(buf.view(np.float32))
    rig.air.cells(77, A, F, 0, d, cell, T * cell, taps=taps_d)
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.complex64).reshape(A, T, cell)
    want = am.AirModel(oraclebind.Oracle(sps)).cells(77, x, taps=taps)
    bad = sum(int((words(got[a, t, :len(x[a][t])]) != words(want[a][t])).sum()) for a in range(A) for t in range(T))
    print("sps %d: %d words differ" % (sps, bad))
    assert bad == 0


def test_bad_arguments(rig):
    import ctypes as C
    pkg, ctx, L = rig.pkg, rig.ctx, rig.ctx.L
    air = pkg.Air(ctx, 8)
    dop, taps = dev_u32(np.zeros(24, np.uint32)), dev(np.zeros((A * 8 * F * 8, 2), np.float32))
    words32, steps32 = dev(np.zeros(24 * 12 * 33, np.int32)), dev(np.zeros(24 * 12 * 33, np.int32))
    fade = lambda fn=0, A_=A, F_=F, n=24, d=dop.data_ptr(), o=taps.data_ptr(): L.trxsig_air_fade(air.h, fn, A_, F_, 0, None, n, d, o)
    params = lambda n=24, d=dop.data_ptr(), p=words32.data_ptr(), s=steps32.data_ptr(): L.trxsig_air_fade_params(air.h, 0, n, d, p, s)
    assert fade() == EINVAL and params() == EINVAL              # no profile set
    assert b"no profile" in L.trxsig_last_error(ctx.h)
    i32, f32 = lambda v: (C.c_int32 * len(v))(*v), lambda v: (C.c_float * len(v))(*v)
    prof = lambda P=2, d=i32([0, 500]), w=f32([0.5, 0.5]), ls=None, lc=None, S=4, n=8, c=0: L.trxsig_air_fade_profile(air.h, P, d, w, ls, lc, S, n, c)
    for kw in (dict(P=0), dict(P=13), dict(S=0), dict(S=33), dict(n=0), dict(n=9), dict(c=-1), dict(c=9), dict(d=None), dict(w=None),
               dict(d=i32([0, -1])), dict(d=i32([0, 1000001])), dict(w=f32([0.5, -0.1])), dict(w=f32([0.5, float("nan")])),
               dict(w=f32([0.5, float("inf")])), dict(ls=f32([0.0, 1.5])), dict(ls=f32([-0.1, 0])), dict(lc=i32([Q23 + 1, 0])),
               dict(lc=i32([0, -Q23 - 1]))):
        assert prof(**kw) == EINVAL, kw
    assert fade() == EINVAL                                     # the refused profiles set nothing
    assert prof() == 0 and prof(ls=f32([1.0, 0.0]), lc=i32([Q23, -Q23])) == 0 and prof(P=1, S=1, n=1, c=8) == 0 and prof() == 0
    assert fade() == 0 and params() == 0
    assert fade(fn=-1) == EINVAL and fade(fn=am.HYPER) == EINVAL and fade(fn=am.HYPER - 1) == 0
    assert fade(F_=0) == EINVAL and fade(F_=(1 << 24) + 1) == EINVAL and fade(A_=0) == EINVAL and fade(A_=1025) == EINVAL
    assert fade(n=0) == EINVAL and fade(n=-5) == EINVAL and fade(d=None) == EINVAL and fade(o=None) == EINVAL
    assert params(n=0) == EINVAL and params(n=(1 << 24) + 1) == EINVAL and params(d=None) == EINVAL and params(p=None) == EINVAL and params(s=None) == EINVAL
    cols = lambda n, v: L.trxsig_air_fade_columns(air.h, n, v)
    assert cols(0, i32([0])) == EINVAL and cols(1025, i32([0] * 1025)) == EINVAL and cols(2, None) == EINVAL
    assert cols(2, i32([0, 10 ** 7 + 1])) == EINVAL and cols(2, i32([-(10 ** 7), 10 ** 7])) == 0
    assert fade(A_=2) == 0 and fade(A_=3) == EINVAL            # more columns than were set
    assert cols(3, i32([0, 200, 400])) == 0 and fade() == 0
    ctx.synchronize()
    air.destroy()
