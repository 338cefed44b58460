"""GPU tests of the air (include/trxsig_air.h) against tests/air_model.py, at sps 1 and 4.

  signal path   raw words equal to the model with no noise: 2 ARFCNs x 2 frames, channels of 1, 2 and 32 taps and none, steps
                zero and not, phases that wrap past 2^32, both stride nestings, in place, accumulated onto a buffer that is not
                zero, cells holding NaN samples, the guard words round every cell untouched
  noise         zeros in: every component within 1e-5 sigma of the float64 model (the header's bar); sigma = 0 and no sigma
                leave the signal's words as they are; cells(x, sigma) = float32(cells(x) + cells(0, sigma)) word for word
  split         one call equals two, bit for bit, in both forms -- the cell form across the hyperframe's wrap
  stream form   3 handsets on 2 carriers of 2 frames + 2 slots, one tile plus 5 samples; cuts at 0, inside slot 0 and running
                past the stream's end; delays -1.5, 0.005 (no sinc), 3.0 and 7.3: words equal without noise, the noise bar with
  refusals      the argument rules of the header that need a live object, and the context kept alive
  downlink loop L1Tx -> modulate -> stream -> L1Acq.search -> L1MsRx: 8 handsets at 20 dB reach state 15 inside the truth bounds
  uplink loop   L1Ms -> radiate -> cells (30 dB, 1e-4 turn per sample) -> TrxGroup.pull -> L1Rx: every payload and RA back"""
import numpy as np
import pytest

import _pkg
import air_model as am
import oraclebind

pytestmark = pytest.mark.gpu
EINVAL = -1
GUARD = np.complex64(complex(-777.25, 123.5))
TILE = 512                                                  # TRX_AIR_TILE


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_c(a):
    return dev(np.ascontiguousarray(a, np.complex64).view(np.float32).reshape(np.shape(a) + (2,)))


def dev_u32(a):
    return dev(np.ascontiguousarray(a, np.uint32).view(np.int32))


def words(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


class Layout:
    """where cell (a, t) lies in a flat buffer: `lead` samples, then cells of 157 sps + gap in either nesting"""

    def __init__(self, A, T, sps, nest, gap=3, lead=5):
        self.A, self.T, self.sps, self.lead = A, T, sps, lead
        cell = 157 * sps + gap
        self.slot, self.arfcn = (cell, T * cell) if nest == "arfcn-major" else (A * cell, cell)
        self.total = lead + A * T * cell

    def at(self, a, t):
        return self.lead + t * self.slot + a * self.arfcn

    def pack(self, cells):
        buf = np.full(self.total, GUARD, np.complex64)
        for a in range(self.A):
            for t in range(self.T):
                buf[self.at(a, t):self.at(a, t) + len(cells[a][t])] = cells[a][t]
        return buf

    def unpack(self, buf):
        return [[buf[self.at(a, t):self.at(a, t) + am.cell_len(t, self.sps)].copy() for t in range(self.T)] for a in range(self.A)]


class Rig:
    def __init__(self, pkg, sps):
        self.pkg, self.sps = pkg, sps
        self.ctx = pkg.TrxSig(sps, 0)
        self.ctx.use_torch_stream()
        self.air = pkg.Air(self.ctx)
        self.model = am.AirModel(oraclebind.Oracle(sps))

    def cells(self, fn, F, lay, buf, seed=0, out=None, out_lay=None, taps=None, step=None, phase=None, sigma=None, accumulate=False):
        """buf / out: host complex64 buffers in lay / out_lay (out None: in place) -> the output buffer after the call"""
        import torch
        d_in = dev(buf.view(np.float32))
        d_out = d_in if out is None else dev(out.view(np.float32))
        ol = lay if out is None else out_lay
        kw = dict(taps=None if taps is None else dev_c(np.array(taps, np.complex64)),
                  step=None if step is None else dev_u32(step), phase=None if phase is None else dev_u32(phase),
                  sigma=None if sigma is None else dev(np.asarray(sigma, np.float32)))
        self.air.cells(fn, lay.A, F, seed, d_in.data_ptr() + 8 * lay.lead, lay.slot, lay.arfcn,
                       d_out.data_ptr() + 8 * ol.lead, ol.slot, ol.arfcn, accumulate=accumulate, **kw)
        torch.cuda.synchronize()
        if out is not None:
            assert np.array_equal(d_in.cpu().numpy().view(np.uint32), buf.view(np.uint32)), "the input was written"
        return d_out.cpu().numpy().view(np.complex64).ravel()

    def stream(self, lay, buf, n_cells, seed, length, arfcn, cut, stride=None, **kw):
        import torch
        H = len(arfcn)
        stride = stride or length + 3
        d_in = dev(buf.view(np.float32))
        out = torch.from_numpy(np.full((H, stride), GUARD, np.complex64).view(np.float32)).cuda()
        conv = dict(delay=lambda v: dev(np.asarray(v, np.float32)), sigma=lambda v: dev(np.asarray(v, np.float32)), step=dev_u32,
                    phase=dev_u32, n0=dev_u32, gain=lambda v: dev_c(np.asarray(v, np.complex64)))
        t = {k: conv[k](v) for k, v in kw.items() if v is not None}
        self.air.stream(lay.A, n_cells, seed, d_in.data_ptr() + 8 * lay.lead, lay.slot, lay.arfcn, out, stride, length,
                        dev(np.asarray(arfcn, np.int32)), dev(np.asarray(cut, np.int64)), **t)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.complex64).reshape(H, stride)
        assert (got[:, length:] == GUARD).all(), "written past len"
        return got[:, :length].copy()


@pytest.fixture(scope="module", params=[1, 4])
def rig(request, pkg):
    return Rig(pkg, request.param)


def per_cell(rng, A, T, Lh):
    taps = (rng.standard_normal((A, T, Lh)) + 1j * rng.standard_normal((A, T, Lh))).astype(np.complex64) if Lh else None
    step = rng.integers(0, 1 << 32, (A, T)).astype(np.uint32)
    step[:, ::5] = 0                                           # some cells with a start phase and no step
    step[:, 1::5] >>= 12                                       # ... with a small one
    phase = rng.integers(0, 1 << 32, (A, T)).astype(np.uint32)
    phase[:, ::3] = 0xffffff00 + rng.integers(0, 256, phase[:, ::3].shape)   # wraps within the first samples
    return taps, step, phase


CASES = [  # Lh, with an offset, nesting, in place, accumulate, NaN samples
    (0, True, "arfcn-major", False, False, False),
    (1, False, "slot-major", True, False, False),
    (2, True, "arfcn-major", False, True, False),
    (32, True, "slot-major", False, False, True),
    (32, False, "arfcn-major", True, True, False),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "Lh%d-%s%s%s%s%s" % (c[0], c[2], "-offset" * c[1], "-inplace" * c[3], "-acc" * c[4], "-nan" * c[5]))
def test_signal_path_words(rig, case):
    Lh, offset, nest, inplace, acc, nan = case
    sps, A, F = rig.sps, 2, 2
    T = 8 * F
    rng = np.random.default_rng(100 + Lh + sps)
    x = am.random_cells(rng, A, T, sps)
    x[0][3][:] = 0                                              # an empty cell
    if nan:
        x[1][5][7] = np.nan; x[0][8][-1] = complex(1.0, np.nan); x[1][12][0] = np.nan
    taps, step, phase = per_cell(rng, A, T, Lh)
    if not offset:
        step = phase = None
    elif Lh == 2:
        step = np.zeros_like(step)                               # the stage runs with a step of zero everywhere
    lay = Layout(A, T, sps, nest)
    buf = lay.pack(x)
    if inplace:
        base = x if acc else None
        got = rig.cells(7, F, lay, buf, taps=taps, step=step, phase=phase, accumulate=acc)
    else:
        ol = Layout(A, T, sps, "slot-major" if nest == "arfcn-major" else "arfcn-major", gap=1, lead=2)
        prior = am.random_cells(rng, A, T, sps, 10.0)
        out = ol.pack(prior)
        base = prior if acc else None
        got = rig.cells(7, F, lay, buf, out=out, out_lay=ol, taps=taps, step=step, phase=phase, accumulate=acc)
        lay = ol
    want = lay.pack(rig.model.cells(7, x, 0, taps, step, phase, None, base))
    bad = np.flatnonzero(words(got).reshape(-1, 2) != words(want).reshape(-1, 2))
    print("sps %d %s: %d words differ of %d" % (sps, case, len(bad), 2 * len(want)))
    if len(bad):
        i = bad[0] // 2
        print("first at sample %d: got %r (%s) want %r (%s)" % (i, got[i], words(got[i:i + 1]), want[i], words(want[i:i + 1])))
    assert len(bad) == 0
    if nan:
        cells = lay.unpack(got)
        assert np.isnan(cells[1][5][7:7 + Lh]).all() and not np.isnan(cells[1][5][:7]).any() and not np.isnan(cells[1][4]).any()


def noise_setup(rig, seed):
    sps, A, F = rig.sps, 2, 2
    T = 8 * F
    rng = np.random.default_rng(seed)
    sigma = rng.uniform(0.05, 4.0, (A, T)).astype(np.float32)
    sigma[1, 2] = 0.0
    sigma[0, 9] = np.float32(3.0e4)
    return sps, A, F, T, rng, sigma, Layout(A, T, sps, "arfcn-major")


def test_noise_alone(rig):
    sps, A, F, T, rng, sigma, lay = noise_setup(rig, 5)
    fn, seed = 1234567, 0x0123456789abcdef
    zeros = [[np.zeros(am.cell_len(t, sps), np.complex64) for t in range(T)] for _ in range(A)]
    got = lay.unpack(rig.cells(fn, F, lay, lay.pack(zeros), seed=seed, sigma=sigma))
    worst, big = 0.0, 0.0
    for a in range(A):
        for t in range(T):
            g = am.cell_gauss(seed, fn, t, a, am.cell_len(t, sps))
            s = float(sigma[a, t])
            if s == 0:
                assert not words(got[a][t]).any()
                continue
            e = got[a][t].astype(np.complex128) / s - g
            worst = max(worst, np.abs(e.real).max(), np.abs(e.imag).max())
            big = max(big, np.abs(g).max())
    print("sps %d: worst |device - float64 model| = %.3e sigma (bar 1e-5); largest |g| %.2f" % (sps, worst, big))
    assert worst <= 1e-5
    # the noise is the counter's, not the launch's: other strides, the same values
    other = Layout(A, T, sps, "slot-major", gap=9, lead=1)
    again = other.unpack(rig.cells(fn, F, other, other.pack(zeros), seed=seed, sigma=sigma))
    assert all(np.array_equal(words(p), words(q)) for r, s in zip(got, again) for p, q in zip(r, s))
    # another seed word, another frame, another ARFCN: other values
    for kw in (dict(seed=seed ^ 1), dict(seed=seed ^ (1 << 40)), dict(fn=fn + 1)):
        o = lay.unpack(rig.cells(kw.get("fn", fn), F, lay, lay.pack(zeros), seed=kw.get("seed", seed), sigma=sigma))
        assert not np.array_equal(o[0][0], got[0][0])
    assert not np.array_equal(got[0][1] / sigma[0, 1], got[1][1] / sigma[1, 1])


def test_sigma_zero_and_composition(rig):
    sps, A, F, T, rng, sigma, lay = noise_setup(rig, 6)
    x = am.random_cells(rng, A, T, sps)
    taps, step, phase = per_cell(rng, A, T, 5)
    kw = dict(taps=taps, step=step, phase=phase)
    plain = rig.cells(99, F, lay, lay.pack(x), **kw)
    zero = rig.cells(99, F, lay, lay.pack(x), sigma=np.zeros((A, T), np.float32), **kw)
    assert np.array_equal(words(plain), words(zero))
    assert np.array_equal(words(rig.cells(99, F, lay, lay.pack(x))), words(lay.pack(x)))     # no stage at all: a copy
    zeros = [[np.zeros_like(c) for c in r] for r in x]
    noise = rig.cells(99, F, lay, lay.pack(zeros), seed=3, sigma=sigma)
    both = rig.cells(99, F, lay, lay.pack(x), seed=3, sigma=sigma, **kw)
    for (a, t) in [(a, t) for a in range(A) for t in range(T)]:
        p, n, b = (lay.unpack(v)[a][t] for v in (plain, noise, both))
        s = np.empty_like(p)
        s.real = p.real + n.real
        s.imag = p.imag + n.imag
        assert np.array_equal(words(s), words(b)), (a, t)
    assert (both == GUARD).sum() == (plain == GUARD).sum()


def test_cells_split_equals_whole(rig):
    sps, A, F = rig.sps, 2, 4
    T = 8 * F
    rng = np.random.default_rng(8)
    x = am.random_cells(rng, A, T, sps)
    taps, step, phase = per_cell(rng, A, T, 3)
    sigma = rng.uniform(0.1, 1.0, (A, T)).astype(np.float32)
    fn = am.HYPER - 2
    lay = Layout(A, T, sps, "slot-major")
    whole = lay.unpack(rig.cells(fn, F, lay, lay.pack(x), seed=11, taps=taps, step=step, phase=phase, sigma=sigma))
    half = Layout(A, T // 2, sps, "slot-major")
    parts = []
    for k, f in enumerate((fn, 0)):
        sl = slice(16 * k, 16 * k + 16)
        xs = [r[sl] for r in x]
        parts.append(half.unpack(rig.cells(f, 2, half, half.pack(xs), seed=11, taps=taps[:, sl], step=step[:, sl], phase=phase[:, sl],
                                           sigma=sigma[:, sl])))
    for a in range(A):
        for t in range(T):
            assert np.array_equal(words(whole[a][t]), words(parts[t // 16][a][t % 16])), (a, t)
    assert not np.array_equal(whole[0][0], whole[0][16][:len(whole[0][0])])


def stream_setup(rig):
    sps = rig.sps
    rng = np.random.default_rng(20 + sps)
    n_cells = 18                                               # 2 frames + 2 slots
    x = am.random_cells(rng, 2, n_cells, sps)
    Ls = sum(len(c) for c in x[0])
    lay = Layout(2, n_cells, sps, "arfcn-major")
    return sps, rng, n_cells, x, Ls, lay, lay.pack(x)


@pytest.mark.parametrize("delay", [[-1.5, 0.005, 3.0], [7.3, 0.0, -0.004]], ids=["a", "b"])
def test_stream_words_and_noise(rig, delay):
    sps, rng, n_cells, x, Ls, lay, buf = stream_setup(rig)
    L = TILE + 5
    arfcn, cut = [1, 0, 1], [0, 37 * sps // 2 + 3, Ls - 200]
    step, phase = [0x01234567, 0, 0xfedcba98], [0xffffff80, 0x80000000, 1]
    gain = [0.7 - 0.2j, 1.0, -3.0j]
    if delay[0] > 7:                                           # once: the optional arrays left out
        assert np.array_equal(words(rig.stream(lay, buf, n_cells, 1, L, arfcn, cut, gain=gain)),
                              words(rig.model.stream(x, 1, arfcn, cut, L, gain=gain)))
        bare = rig.stream(lay, buf, n_cells, 1, L, arfcn, cut)
        assert np.array_equal(words(bare), words(rig.model.stream(x, 1, arfcn, cut, L)))
        assert np.array_equal(words(bare[0]), words(np.concatenate(x[1])[:L]))
    plain = rig.stream(lay, buf, n_cells, 1, L, arfcn, cut, delay=delay, step=step, phase=phase, gain=gain)
    want = rig.model.stream(x, 1, arfcn, cut, L, delay, step, phase, gain)
    bad = np.argwhere(words(plain) != words(want))
    print("sps %d delays %s: %d words differ" % (sps, delay, len(bad)), bad[:4])
    assert len(bad) == 0
    assert not plain[2, 200:].any() and plain[2, 100:190].all()   # past the stream's end: zeros
    sigma, n0 = [0.1, 2.5, 0.7], [0, 0xfffffff1, 12345]
    noisy = rig.stream(lay, buf, n_cells, 0xabcdef0123, L, arfcn, cut, delay=delay, step=step, phase=phase, gain=gain, sigma=sigma, n0=n0)
    for h in range(3):
        g = am.stream_gauss(0xabcdef0123, h, n0[h], L)
        exact = want[h].astype(np.complex128) + float(np.float32(sigma[h])) * g
        e = noisy[h].astype(np.complex128) - exact
        # the device's g within 1e-5 (the header's bar), and the one rounding of the float32 sum
        tol = 1e-5 * sigma[h] + 2.0 ** -24 * np.maximum(np.abs(exact.real), np.abs(exact.imag))
        print("handset %d: worst error / tolerance %.3f" % (h, max((np.abs(e.real) / tol).max(), (np.abs(e.imag) / tol).max())))
        assert (np.abs(e.real) <= tol).all() and (np.abs(e.imag) <= tol).all()
    # a carrier that does not exist is silence; noise alone still arrives
    lost = rig.stream(lay, buf, n_cells, 5, L, [2, -1, 0], cut, delay=delay, sigma=[0.0, 1.0, 0.0])
    assert not lost[0].any() and lost[1].all() and np.array_equal(words(lost[2]), words(rig.model.stream(x, 5, [0], cut[2:], L, delay[2:])[0]))


def test_stream_split_equals_whole(rig):
    sps, rng, n_cells, x, Ls, lay, buf = stream_setup(rig)
    L, L1 = 2 * TILE + 77, TILE - 31
    arfcn, cut, delay = [0, 1, 1], [-40, 5, Ls - 900], [0.31, -2.0, 12.5]
    step, phase, n0 = [0x00100001, 0xf0000003, 7], [0, 0xfffffffe, 99], [1, 0xffffff00, 6]
    gain, sigma = [1.0, 0.5j, -1.5], [0.2, 0.4, 0.0]
    kw = dict(delay=delay, gain=gain, sigma=sigma, step=step)
    whole = rig.stream(lay, buf, n_cells, 77, L, arfcn, cut, phase=phase, n0=n0, **kw)
    adv = lambda v, k: [(p + q * L1) & 0xffffffff for p, q in zip(v, k)]
    a = rig.stream(lay, buf, n_cells, 77, L1, arfcn, cut, phase=phase, n0=n0, **kw)
    b = rig.stream(lay, buf, n_cells, 77, L - L1, arfcn, [c + L1 for c in cut], phase=adv(phase, step), n0=adv(n0, [1, 1, 1]), **kw)
    assert np.array_equal(words(whole), words(np.concatenate([a, b], axis=1)))


def test_bad_arguments_and_lifetime(rig):
    import ctypes as C
    pkg, ctx, L, sps = rig.pkg, rig.ctx, rig.ctx.L, rig.sps
    before = L.trxsig_live_children(ctx.h)
    air = pkg.Air(ctx, 4)
    assert L.trxsig_live_children(ctx.h) == before + 1
    for bad in (0, 33, -1):
        h = C.c_void_p()
        assert L.trxsig_air_create(C.byref(h), ctx.h, bad) == EINVAL and not h.value
    cell, A, F = 157 * sps, 2, 1
    T = 8 * F
    d = dev(np.zeros(2 * 2 * A * T * cell + 64, np.float32))
    p, q = d.data_ptr(), d.data_ptr() + 8 * A * T * cell
    taps = dev(np.zeros((A, T, 5, 2), np.float32))
    par = pkg.AirCellParams()
    cells = lambda fn, A_, F_, i, ss, sa, o, os_, oa, pr=par: L.trxsig_air_cells(air.h, fn, A_, F_, 0, i, ss, sa, C.byref(pr) if pr else None, o, os_, oa, 0)
    assert cells(0, A, F, p, cell, T * cell, q, cell, T * cell) == 0
    assert cells(0, A, F, p, cell, T * cell, p, cell, T * cell) == 0                      # in place
    assert cells(0, A, F, p, A * cell, cell, q, cell, T * cell) == 0                      # the other nesting
    assert cells(0, A, 0, p, cell, T * cell, q, cell, T * cell) == EINVAL and cells(0, A, -1, p, cell, T * cell, q, cell, T * cell) == EINVAL
    assert cells(-1, A, F, p, cell, T * cell, q, cell, T * cell) == EINVAL and cells(am.HYPER, A, F, p, cell, T * cell, q, cell, T * cell) == EINVAL
    assert cells(am.HYPER - 1, A, F, p, cell, T * cell, q, cell, T * cell) == 0
    assert cells(0, 0, F, p, cell, T * cell, q, cell, T * cell) == EINVAL
    assert cells(0, A, F, p, cell - 1, T * cell, q, cell, T * cell) == EINVAL            # cells overlap
    assert cells(0, A, F, p, cell, T * cell - 1, q, cell, T * cell) == EINVAL
    assert cells(0, A, F, p, cell, T * cell, q, cell, cell) == EINVAL
    assert cells(0, A, F, p, cell, T * cell, p + 8, cell, T * cell) == EINVAL            # overlapping without being identical
    assert cells(0, A, F, p, cell, T * cell, p, A * cell, cell) == EINVAL                # the same base, other strides
    assert cells(0, A, F, None, cell, T * cell, q, cell, T * cell) == EINVAL and cells(0, A, F, p, cell, T * cell, None, cell, T * cell) == EINVAL
    assert cells(0, A, F, p, cell, T * cell, q, cell, T * cell, None) == EINVAL
    for n, rc in ((0, EINVAL), (5, EINVAL), (4, 0), (1, 0)):                              # the object was made for 4 taps
        pt = pkg.AirCellParams(d_taps=taps.data_ptr(), n_taps=n)
        assert cells(0, A, F, p, cell, T * cell, q, cell, T * cell, pt) == rc, n
    ar, cu = dev(np.zeros(3, np.int32)), dev(np.zeros(3, np.int64))
    sp = pkg.AirStreamParams(n_arfcn=A, d_arfcn=ar.data_ptr(), d_cut=cu.data_ptr())
    n_out = (A * T * cell - 8) // 3
    stream = lambda nc, i, ss, sa, H, ln, o, os_, pr=sp: L.trxsig_air_stream(air.h, nc, 0, i, ss, sa, H, C.byref(pr) if pr else None, ln, o, os_)
    assert stream(T, p, cell, T * cell, 3, 100, q, n_out) == 0
    assert stream(0, p, cell, T * cell, 3, 100, q, n_out) == EINVAL and stream(-3, p, cell, T * cell, 3, 100, q, n_out) == EINVAL
    assert stream(T, p, cell, T * cell, 3, 0, q, n_out) == EINVAL and stream(T, p, cell, T * cell, 3, -5, q, n_out) == EINVAL
    assert stream(T, p, cell, T * cell, 0, 100, q, n_out) == EINVAL and stream(T, p, cell, T * cell, 3, 100, q, 99) == EINVAL
    assert stream(T, p, cell - 1, T * cell, 3, 100, q, n_out) == EINVAL and stream(T, p, cell, T * cell, 3, 100, p + 800, n_out) == EINVAL
    assert stream(2 ** 31 // (157 * sps) + 1, p, cell, 2 ** 40, 3, 100, q, n_out) == EINVAL
    assert stream(T, p, cell, T * cell, 3, 100, q, n_out, None) == EINVAL
    assert stream(T, p, cell, T * cell, 3, 100, q, n_out, pkg.AirStreamParams(n_arfcn=A, d_arfcn=ar.data_ptr())) == EINVAL
    ctx.synchronize()
    assert not d.cpu().numpy().any()                         # zeros in, nothing applied: the refused calls wrote nothing either
    air.destroy()
    assert L.trxsig_live_children(ctx.h) == before


def test_downlink_loop(rig):
    """L1Tx.encode -> trxsig_modulate_batch into cells -> Air.stream (8 handsets on C0: random cut inside the first multiframe,
    delay in [0, 1), offset within +-0.02 cycle / symbol, 20 dB) -> L1Acq.search -> each handset's SCH row through
    L1MsRx.decode.  Every handset reaches state 15 with the true FN and BSIC, the grid within 0.25 sample and the offset within
    2e-3 cycle / symbol (the bounds of tests/test_gpu_l1acq.py's 20 dB streams), and its row syncs in the decoder.  The case is
    tests/air_loops.py's; tests/test_air_model.py holds the model and the reference's detectors to the same bounds on it."""
    import torch
    import air_loops as al
    import fectxbind
    pkg, ctx, sps = rig.pkg, rig.ctx, rig.sps
    case = al.downlink_case(sps, fectxbind.FecTxOracle())
    comb, F, H, n = case["mux"].comb, case["F"], case["H"], case["n"]
    A, T = comb.shape[0], 8 * F
    l1 = pkg.L1Tx(ctx, comb, case["bsic"], case["band"])
    l1.set_si(case["mux"].si)
    l1.encode(case["fn0"], F, **{k: dev(v) for k, v in case["grids"].items()})
    enc = l1.collect(state=False)
    assert np.array_equal(enc["what"], case["enc"]["what"]) and np.array_equal(enc["bits"], case["enc"]["bits"])
    sent = np.argwhere(enc["what"] != 0)                       # (a, t)
    cellw = 157 * sps + 3
    cells = torch.zeros(A * T * cellw, 2, dtype=torch.float32, device="cuda")
    ctx.modulate(dev(enc["bits"][enc["what"] != 0]), dev((8 + (sent[:, 1] % 4 == 0)).astype(np.int32)), cells,
                 dev(((sent[:, 0] * T + sent[:, 1]) * cellw).astype(np.int32)))
    stride = n + 7
    out = torch.zeros(H, stride, 2, dtype=torch.float32, device="cuda")
    rig.air.stream(A, T, case["seed"], cells, cellw, T * cellw, out, stride, n, dev(np.zeros(H, np.int32)),
                   dev(np.asarray(case["cut"], np.int64)), delay=dev(case["delay"]), step=dev_u32(case["step"]),
                   phase=dev_u32(case["phase"]), gain=dev_c(case["gain"]), sigma=dev(case["sigma"]), n0=dev_u32(case["n0"]))
    acq = pkg.L1Acq(ctx, H, n)
    acq.search(out, stride, n, H)
    g = acq.collect()
    worst_t = worst_f = 0.0
    for h in range(H):
        dt, df = al.check_handset(case, h, int(g["state"][h]), int(g["bsic"][h]), int(g["rfn"][h]),
                                  int(g["sch_w0"][h]) + float(g["sch_toa"][h]), float(g["arg"][h]) / (2 * np.pi))
        worst_t, worst_f = max(worst_t, dt), max(worst_f, df)
    print("sps %d: worst timing error %.3f sample, worst offset error %.2e cycle / symbol" % (sps, worst_t, worst_f))
    assert worst_t <= al.MAX_TIMING and worst_f <= al.MAX_OFFSET
    # the SCH rows through the handsets' decoder: one frame each, the row of the search in TN 0 of ARFCN 0
    valid = torch.full((H,), pkg.F_DETECT, dtype=torch.uint8, device="cuda")
    o = acq.out
    for h in range(H):
        row = np.full((8, A), -1, np.int32)
        row[0, 0] = h
        drow = dev(row)
        res = pkg.TrxGroupResult(n_slots=8, n_arfcn=A, n_rows=H, d_row=drow.data_ptr(), d_valid=valid.data_ptr(), d_flags=None,
                                 d_amp=o.d_sch_amp, d_toa=o.d_sch_toa, d_avgpwr=None, d_threshold=None, d_soft=o.d_soft,
                                 soft_stride=o.soft_stride)
        rx = pkg.L1MsRx(ctx, comb, case["bsic"], case["band"])
        rx.decode(res, int(g["rfn"][h]), True)
        sch = rx.collect(state=False)["sch"]
        assert len(sch["sync"]) == 1 and sch["present"].all() and sch["sync"].all() and int(sch["rfn"][0]) == int(g["rfn"][h]), (h, sch)
        rx.destroy()
    acq.destroy(); l1.destroy()


def test_uplink_loop(pkg):
    """L1Ms.encode -> radiate -> Air.cells in place (noise alone at 30 dB below each burst, a step of 1e-4 turn per sample and a
    random start phase per cell; empty cells get the weakest burst's noise) -> TrxGroup.pull -> L1Rx.decode, on the small plan of
    tests/test_gpu_l1ms.py's closed loop.  Every burst is detected, every XCCH payload and every RA comes back, every TCH frame is
    good.  Why 30 dB: class-2 speech bits are unprotected, so the level must leave the reference itself no doubtful bit.  On the
    CPU (tests/air_loops.py's case through air_model and the oracle's analyzeTrafficBurst / detectRACHBurst + demodulateBurst, run
    once) every one of the 1,138 bursts was detected, no hard bit was wrong, and the smallest |soft - 0.5| was 0.250 (TCH), 0.287
    (XCCH) and 0.292 (access bursts); the condition was 0.1.  (At 20 dB the same run still gave 0.130.)"""
    import torch
    import air_loops as al
    import fec_stream_model as fsm
    import fectxbind
    import l1_ms_model as lms
    case = al.uplink_case(fectxbind.FecTxOracle())
    sps, A, F, T, fn0, bsic, band, comb = (case[k] for k in ("sps", "A", "F", "T", "fn0", "bsic", "band", "comb"))
    model, g, m = case["model"], case["grids"], case["m"]
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    ms = pkg.L1Ms(ctx, comb, bsic, band)
    for i, p, t in case["phy"]:
        ms.set_phy(i, p, t)
    ms.encode(fn0, F, **{k: dev(v) for k, v in g.items()})
    r = ms.collect(state=False)
    assert np.array_equal(r["what"], m["what"]) and np.array_equal(r["bits"], m["bits"])
    cell = 160 * sps
    buf = torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda")
    ms.radiate(buf, A * cell, cell, tch_gain=dev_c(case["gain"][0]), xcch_gain=dev_c(case["gain"][1]), rach_gain=dev_c(case["gain"][2]),
               tch_delay=dev(case["delay"][0]), xcch_delay=dev(case["delay"][1]), rach_delay=dev(case["delay"][2]),
               amp_of_power=dev(np.ones(41, np.float32)))
    air = pkg.Air(ctx, 1)
    air.cells(fn0, A, F, case["seed"], buf, A * cell, cell, step=dev_u32(case["step"]), phase=dev_u32(case["phase"]),
              sigma=dev(case["sigma"]))
    rx_cells = buf.cpu().numpy().view(np.complex64).reshape(T, A, cell)
    assert not rx_cells[:, :, 157 * sps:].any() and rx_cells[1, 0, :156 * sps].all() and not rx_cells[1, 0, 156 * sps:].any()
    grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn0, 0))
    for a in range(A):
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % (bsic & 7)] + \
                   ["CMD SETSLOT %d %d" % (tn, comb[a, tn]) for tn in range(8)] + ["CMD POWERON"]:
            grp.control(a, cmd)
    res = grp.pull(buf.data_ptr(), A * cell, cell, fn0, 0, T)
    grp.sync()
    rx = pkg.L1Rx(ctx, comb, bsic, band)
    rx.decode(res, fn0)
    got = rx.collect()
    col = grp.collect()
    missed = [(t, a) for t, a in np.argwhere(m["what"].T != 0) if not col["valid"][t, a]]
    assert not missed, ("a burst was not detected", missed[:5])
    # every TCH frame good (stream block b carries encoded block b - 1), every FACCH frame back
    n_tch = 0
    for s in range(len(model.ch[lms.TCH])):
        for b in range(1, g["tch_kind"].shape[1]):
            kind, pl = g["tch_kind"][s, b - 1], g["tch_payload"][s, b - 1]
            if kind == pkg.TCH_SPEECH:
                assert got["tch_status"][s, b] == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(got["tch"][s, b], pl), (s, b)
            else:
                assert got["tch_status"][s, b] & fsm.FACCH_OK and np.array_equal(got["facch"][s, b], pl[:23]), (s, b)
            n_tch += 1
    n_x = 0
    for s, c in enumerate(model.ch[lms.XCCH]):
        w = model.walk(c.m, fn0, F)
        b = 0
        for j, (k, B) in enumerate(w):
            if B != 0:
                continue
            if j + 3 < len(w) and g["xcch_kind"][s, b] == 1:
                want = g["xcch_payload"][s, b].copy()
                if c.sacch:
                    want[0], want[1] = lms.lmm.encode_power(band, c.power) & 31, c.ta
                jb = list(got["xcch_fn"][s]).index((fn0 + w[j + 3][0]) % al.HYPER)
                assert got["xcch_status"][s, jb] == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(got["xcch"][s, jb], want), (s, b)
                n_x += 1
            b += 1
    assert n_tch > 100 and n_x > 40
    # every RA: the access bursts sent with the cell's BSIC come back, in order; one with another BSIC is refused
    walk = model.walk(model.ch[lms.RACH][0].m, fn0, F)
    sent_r = [((fn0 + k) % al.HYPER, int(g["rach_ra"][j]), int(g["rach_bsic"][j])) for j, (k, _) in enumerate(walk) if g["rach_kind"][j] == 1]
    rr = got["rach"]
    heard = {int(f): (bool(ok), int(v)) for f, ok, v in zip(rr["fn"], rr["ok"], rr["ra"])}
    for f, ra, b in sent_r:
        assert f in heard and heard[f] == ((b == bsic), ra if b == bsic else 0), (f, ra, b, heard.get(f))
    assert sum(b == bsic for _, _, b in sent_r) > 20
    ms.destroy(); rx.destroy(); air.destroy(); grp.close(); ctx.close()
