"""GPU parity of the mobile-side uplink L1 (trxsig_l1ms.h) against its literal CPU model (tests/l1_ms_model.py) and against the
library's own primitives: random plans with open / close / set_phy at the superframe and hyperframe wraps; random splits of one
span; all 256 x 64 access bursts through the RACH decoder; radiate against modulate -> delayVector -> scaleVector, bit for bit;
the closed loop L1Ms -> radiate -> TrxGroup.pull -> L1Rx; the orders round trip L1Tx -> L1Ms -> L1Rx; the bad-input rules; a call
past one launch slice.  Every comparison is exact."""
import numpy as np
import pytest

import _pkg
import fec_stream_model as fsm
import l1_demux_model as ldm
import l1_ms_model as lms

pytestmark = pytest.mark.gpu
HYPER = lms.HYPERFRAME
EINVAL = -1


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.TrxSig(4, 0)
    c.use_torch_stream()
    return c


@pytest.fixture(scope="module")
def oracle():
    import fectxbind
    return fectxbind.FecTxOracle()


@pytest.fixture(scope="module")
def prims():
    return fsm.Prims()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_plan(rng, A, c5=True):
    comb = rng.choice(np.array([0, 1, 1, 7], np.uint8), (A, 8))
    if c5:
        comb[0, 0] = 5
    return comb


def gpu_call(ms, fn, F, g, sibling=None, state=True):
    t = {k: dev(v) for k, v in g.items()}
    ms.encode(fn % HYPER, F, sibling=sibling, **t)
    r = ms.collect(state=state)
    r["_keep"] = t
    return r


KEYS = ("what", "bits", "ms_power", "ms_ta", "tch_state", "xcch_state")


def assert_same(r, m, what=""):
    assert np.array_equal(r["what"], m["what"]), (what, np.argwhere(r["what"] != m["what"])[:8])
    bad = np.argwhere((r["bits"] != m["bits"]).any(-1))
    assert len(bad) == 0, (what, bad[:8], r["what"][tuple(bad[0])] if len(bad) else None)
    for k in KEYS[2:]:
        assert np.array_equal(r[k], m[k]), (what, k, np.argwhere(r[k] != m[k])[:8])


def random_control(rng, ms, model):
    """open / close / set_phy of random channels, on the object and on the model"""
    for _ in range(4):
        cls = int(rng.integers(0, 2))
        n = ms.channels(cls)
        if not n:
            continue
        i = int(rng.integers(0, n))
        op = rng.random()
        if op < 0.3:
            ms.close(cls, i); model.close(cls, i)
        elif op < 0.6:
            ms.open(cls, i); model.open(cls, i)
        elif cls == lms.XCCH and model.ch[cls][i].sacch:
            p, t = int(rng.integers(0, 41)), int(rng.integers(0, 64))
            ms.set_phy(i, p, t); model.set_phy(i, p, t)


# ---- 1 ----
@pytest.mark.parametrize("seed,fn0", [(0, 26 * 51 * 5 - 120), (1, HYPER - 150), (2, 26 * 51 * 2047 - 33)])
def test_random_plans_against_the_model(pkg, ctx, oracle, seed, fn0):
    """A in 1..3, calls of F <= 208 frames across the 26 * 51 superframe wrap and the hyperframe wrap, random open / close /
    set_phy between them: bits, what, the handsets and the channel records equal the model's."""
    rng = np.random.default_rng(500 + seed)
    A = seed + 1
    comb = random_plan(rng, A, c5=seed != 1)
    comb[0, 1], comb[0, 2] = 1, 7                            # every plan has traffic and dedicated control channels
    bsic, band = int(rng.integers(0, 64)), [900, 1800, 1900][seed]
    ms = pkg.L1Ms(ctx, comb, bsic, band)
    model = lms.MsModel(comb, bsic, band, oracle=oracle)
    assert [ms.channels(c) for c in (0, 1, 2)] == [len(model.ch[c]) for c in (0, 1, 2)]
    content = lms.Content(rng)
    fn, seen = fn0, set()
    for call, F in enumerate([int(rng.integers(1, 60)), 208, int(rng.integers(60, 209)), 1]):
        random_control(rng, ms, model)
        g = lms.grids(model, content, fn, F)
        assert ms.grid(fn % HYPER, F) == model.grid(fn, F)
        r = gpu_call(ms, fn, F, g)
        assert_same(r, model.encode(fn, F, **g), (seed, call, fn, F))
        seen |= set(np.unique(r["what"]).tolist())
        fn += F
    assert fn0 < 26 * 51 * ((fn0 // (26 * 51)) + 1) < fn        # the span crossed a superframe boundary
    assert {lms.W_TCH, lms.W_XCCH} <= seen and (seed == 1 or lms.W_ACCESS in seen), seen
    ms.destroy()


# ---- 2 ----
@pytest.mark.parametrize("seed", range(2))
def test_random_splits_equal_one_call(pkg, ctx, seed):
    """One call of F frames against calls split at random frame boundaries (1-frame calls and cuts inside blocks included):
    identical concatenated outputs and state."""
    rng = np.random.default_rng(600 + seed)
    comb = random_plan(rng, int(rng.integers(1, 4)))
    comb[0, 1] = 1
    F = 156
    fn0 = int(rng.integers(0, HYPER - F)) if seed else HYPER - 70
    model = lms.MsModel(comb, 5, oracle=object())           # the walk only: no encoding on the CPU here
    content = lms.Content(rng)
    objs = [pkg.L1Ms(ctx, comb, 5) for _ in range(2)]
    for o in objs:
        o.set_phy(next(i for i, c in enumerate(model.ch[lms.XCCH]) if c.sacch), 11, 42)
        o.close(lms.TCH, 0)
    whole = gpu_call(objs[0], fn0, F, lms.grids(model, content, fn0, F))
    cuts = [0] + sorted(set(rng.choice(np.arange(1, F), 6, replace=False).tolist() + [1, 2])) + [F]
    parts = []
    for lo, hi in zip(cuts, cuts[1:]):
        parts.append(gpu_call(objs[1], fn0 + lo, hi - lo, lms.grids(model, content, fn0 + lo, hi - lo)))
    for k in ("bits", "what"):
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k
    for k in KEYS[2:]:
        assert np.array_equal(parts[-1][k], whole[k]), k
    assert {lms.W_TCH, lms.W_XCCH, lms.W_ACCESS} <= set(np.unique(whole["what"]).tolist())
    for o in objs:
        o.destroy()


# ---- 3 ----
def test_all_access_bursts_through_the_rach_decoder(pkg, ctx):
    """All 256 RA x 64 BSIC, one per RACH frame of a single call, through trxsig_fec_rach_decode_batch: each gives its RA and
    BSIC with the tail bits zero; the fixed part of the burst is GSM 05.02 5.2.7's."""
    import torch
    comb = np.zeros((1, 8), np.uint8)
    comb[0, 0] = 5
    ms = pkg.L1Ms(ctx, comb, 0)
    F = 607 * 51                                             # 27 RACH frames per 51-multiframe: 16,389 entries
    _, nbx, n = ms.grid(1000, F)
    assert n == 607 * 27 >= 256 * 64
    ra = (np.arange(n) % 256).astype(np.uint8)
    bsic = ((np.arange(n) // 256) % 64).astype(np.uint8)
    kind = (np.arange(n) < 256 * 64).astype(np.uint8)
    zx = np.zeros((ms.channels(1), nbx), np.uint8)
    ms.encode(1000, F, xcch_kind=dev(zx), xcch_payload=dev(np.zeros(zx.shape + (23,), np.uint8)), rach_kind=dev(kind),
              rach_ra=dev(ra), rach_bsic=dev(bsic))
    r = ms.collect(state=False)
    on = r["what"][0] == lms.W_ACCESS
    assert on.sum() == 256 * 64 and (r["what"][0][~on] == 0).all()
    b = r["bits"][0][on]
    assert (b[:, :49] == lms.ACCESS_HEAD).all() and not b[:, 85:].any()
    soft = dev(b.astype(np.float32))
    out = [torch.zeros(len(b), dtype=torch.uint8, device="cuda") for _ in range(3)]
    ctx.fec_rach_decode(soft, len(b), *out)
    torch.cuda.synchronize()
    tail_ok, got_bsic, got_ra = [o.cpu().numpy() for o in out]
    assert tail_ok.all() and np.array_equal(got_ra, ra[:len(b)]) and np.array_equal(got_bsic, bsic[:len(b)])
    ms.destroy()


# ---- 4 ----
class Air:
    """Per-channel gains and delays, and a power table, on the host and on the device."""

    def __init__(self, rng, model, n_rach, delay, rach_delay, amp_of_power=None, mag=(300.0, 3000.0)):
        def gains(n):
            g = rng.uniform(mag[0], mag[1], n) * np.exp(2j * np.pi * rng.uniform(size=n))
            return g.astype(np.complex64)
        nt, nx = len(model.ch[lms.TCH]), len(model.ch[lms.XCCH])
        self.gain = [gains(nt), gains(nx), gains(n_rach)]
        self.delay = [delay(nt).astype(np.float32), delay(nx).astype(np.float32), rach_delay(n_rach).astype(np.float32)]
        self.amp = np.ones(41, np.float32) if amp_of_power is None else np.asarray(amp_of_power, np.float32)
        self.t = [dev(g.view(np.float32).reshape(-1, 2)) for g in self.gain] + [dev(d) for d in self.delay] + [dev(self.amp)]

    def kwargs(self):
        t = self.t
        return dict(tch_gain=t[0], xcch_gain=t[1], rach_gain=t[2], tch_delay=t[3], xcch_delay=t[4], rach_delay=t[5],
                    amp_of_power=t[6])

    def cell(self, model, m, a, s, sps):
        """(d, A) of the non-empty slot s of ARFCN a, in float32 as trxsig_l1ms.h writes them"""
        f32 = np.float32
        w, who = int(m["what"][a, s]), int(m["who"][a, s])
        g = self.gain[w - 1][who]
        if w == lms.W_ACCESS:
            return f32(self.delay[2][who] * f32(sps)), g
        hs = model.ch[w - 1][who].handset
        d = f32(f32(self.delay[w - 1][who] - f32(hs.ta)) * f32(sps))
        sc = self.amp[hs.power]
        return d, np.complex64(complex(f32(g.real * sc), f32(g.imag * sc)))


def primitive_chain(c, bits, guard, delays, scales, sps):
    """trxsig_modulate_batch (no gain) -> trxsig_delay_vector_batch -> trxsig_scale_vector_batch: complex64 [B][157 sps]"""
    import torch
    B, pitch = len(bits), 157 * sps
    off = dev((np.arange(B) * pitch).astype(np.int32))
    length = dev(((148 + guard) * sps).astype(np.int32))
    x = torch.zeros(B * pitch, 2, dtype=torch.float32, device="cuda")
    y = torch.zeros_like(x)
    c.modulate(dev(bits), dev(guard.astype(np.int32)), x, off)
    L = c.L
    assert L.trxsig_delay_vector_batch(c.h, x.data_ptr(), off.data_ptr(), length.data_ptr(), B, dev(delays).data_ptr(), 0,
                                       y.data_ptr()) == 0
    sc = dev(np.asarray(scales, np.complex64).view(np.float32).reshape(-1, 2))
    assert L.trxsig_scale_vector_batch(c.h, y.data_ptr(), off.data_ptr(), length.data_ptr(), B, pitch, sc.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    return y.cpu().numpy().reshape(B, pitch, 2)


@pytest.mark.parametrize("sps", [1, 4])
def test_radiate_equals_the_primitive_chain(pkg, oracle, sps):
    """Every cell of a mixed plan against the three primitives on the same bursts, as raw float32 words: 156- and 157-symbol
    slots, empty cells zero, the stride padding and the cells' tails untouched; delays negative, whole, fractional, beyond a
    symbol, one the primitives refuse, access bursts up to 63 symbols late; handsets at several powers and TAs."""
    import torch
    c = pkg.TrxSig(sps, 0)
    c.use_torch_stream()
    rng = np.random.default_rng(700 + sps)
    comb = np.array([[5, 1, 7, 0, 1, 0, 0, 7], [1, 7, 0, 1, 1, 0, 0, 0]], np.uint8)
    A, F, fn0, bsic, band = 2, 60, 51 * 7 + 3, 37, 1900
    ms = pkg.L1Ms(c, comb, bsic, band)
    model = lms.MsModel(comb, bsic, band, oracle=oracle)
    for i, ch in enumerate(model.ch[lms.XCCH]):
        if ch.sacch and i % 3:
            p, t = int(rng.integers(0, 41)), int(rng.integers(0, 64))
            ms.set_phy(i, p, t); model.set_phy(i, p, t)
    g = lms.grids(model, lms.Content(rng, p_none=0.15), fn0, F)
    r = gpu_call(ms, fn0, F, g)
    m = model.encode(fn0, F, **g)
    assert_same(r, m, "encode")

    def delay(n):                                            # about the handset's own TA: whole, fractional, negative, > 1 symbol
        d = rng.choice([0.0, 2.0, -1.0, 0.0025, 0.4, -0.37, 1.75, -3.3, 7.125], n) + rng.choice([0.0, 1e-3], n)
        return d
    air = Air(rng, model, len(g["rach_kind"]), delay, lambda n: rng.uniform(0, 63, n) * (rng.random(n) < 0.8),
              amp_of_power=10.0 ** ((np.arange(41) - 33) / 20.0))
    for cls in (lms.TCH, lms.XCCH):                          # delays are about the handset's TA; one channel per class refused
        ta = np.array([ch.handset.ta for ch in model.ch[cls]], np.float32)
        air.delay[cls] = (air.delay[cls] + ta).astype(np.float32)
        air.delay[cls][1] = 3.0e7
        air.t[3 + cls] = dev(air.delay[cls])
    T, pad = 8 * F, 5
    cellw = 157 * sps + pad
    SENT = np.float32(-777.25)
    buf = torch.full((T, A, cellw, 2), float(SENT), dtype=torch.float32, device="cuda")
    ms.radiate(buf, A * cellw, cellw, **air.kwargs())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    cells = [(a, s) for s in range(T) for a in range(A) if m["what"][a, s]]
    guard = np.array([8 + (s % 4 == 0) for _, s in cells])
    da = [air.cell(model, m, a, s, sps) for a, s in cells]
    want = primitive_chain(c, np.stack([m["bits"][a, s] for a, s in cells]), guard, np.array([d for d, _ in da], np.float32),
                           [x for _, x in da], sps)
    bits32 = lambda v: np.ascontiguousarray(v, np.float32).view(np.uint32)
    n_ref = n_filt = 0
    for i, (a, s) in enumerate(cells):
        N = (148 + guard[i]) * sps
        assert np.array_equal(bits32(got[s, a, :N]), bits32(want[i, :N])), (a, s, m["what"][a, s], da[i])
        n_ref += not np.abs(want[i, :N]).any()
        n_filt += abs(float(da[i][0]) - np.floor(float(da[i][0]))) > 1e-2
    for s in range(T):
        N = (156 + (s % 4 == 0)) * sps
        for a in range(A):
            if not m["what"][a, s]:
                assert not bits32(got[s, a, :N]).any(), (a, s)
            assert (got[s, a, N:] == SENT).all(), (a, s)
    assert n_ref >= 1 and n_filt > 100 and len(cells) - n_filt > 20 and {1, 2, 3} <= set(m["what"].ravel().tolist())
    ms.destroy(); c.close()


# ---- 5, 6: through the air ----
def setup_group(pkg, ctx, comb, tsc, fn0):
    A = comb.shape[0]
    grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn0, 0))
    for a in range(A):
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % tsc] + \
                   ["CMD SETSLOT %d %d" % (tn, comb[a, tn]) for tn in range(8)] + ["CMD POWERON"]:
            grp.control(a, cmd)
    return grp


def radiate_with_noise(ms, air, what, A, F, sps, seed, cell=None):
    """L1Ms.radiate into a zeroed [T][A][160 sps] buffer, then complex noise of sigma 0 or 0.02 |amplitude| on alternate bursts
    (the levels synth.bursts_from_bits(sigmas=(0.0, 0.02)) gives the hand-built closed-loop test), added with torch."""
    import torch
    T = 8 * F
    cell = cell or 160 * sps
    buf = torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda")
    ms.radiate(buf, A * cell, cell, **air.kwargs())
    on = dev(np.ascontiguousarray((what != 0).T))             # [T][A]
    z = torch.view_as_complex(buf)
    mag = z.abs().amax(dim=2)                                 # the burst's envelope peak: about |amplitude|
    sig = torch.where((torch.arange(T * A, device="cuda").reshape(T, A) % 2 == 1) & on, 0.02 * mag, torch.zeros_like(mag))
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = torch.randn(T, A, cell, 2, device="cuda", generator=gen) / np.sqrt(2.0)
    n[:, :, 156 * sps:] = 0
    buf += sig[:, :, None, None] * n
    return buf, cell


def test_closed_loop_by_the_object(pkg, oracle, prims):
    """tests/test_gpu_l1rx.py's hand-built closed loop, done by the object: L1Ms.encode -> radiate -> noise -> TrxGroup.pull with
    the plan's CMD SETSLOT -> L1Rx.decode.  Every burst is detected, the result equals the demultiplexer's model fed
    TrxGroup.collect(), every payload and RA comes back, a wrong-BSIC entry is refused, and the decoder's SACCH power / TA
    are the handsets'."""
    import torch
    sps, A, F, fn0, bsic, band = 4, 2, 208, 26 * 40, 21, 1800
    rng = np.random.default_rng(77)
    comb = np.zeros((A, 8), np.uint8)
    comb[0, :3] = [5, 1, 7]; comb[0, 4] = 1; comb[1, :2] = [1, 7]
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    ms = pkg.L1Ms(ctx, comb, bsic, band)
    model = lms.MsModel(comb, bsic, band, oracle=oracle)
    rxm = ldm.Model(comb, bsic, band=band, prims=prims)
    sacch = [i for i, c in enumerate(model.ch[lms.XCCH]) if c.sacch]
    for i in sacch[::2]:
        p, t = int(rng.integers(0, 41)), int(rng.integers(0, 64))
        ms.set_phy(i, p, t); model.set_phy(i, p, t)
    content = lms.Content(rng, p_none=0.1, speech=True)
    g = lms.grids(model, content, fn0, F)
    r = gpu_call(ms, fn0, F, g)
    m = model.encode(fn0, F, **g)
    assert_same(r, m, "encode")
    # the air: each handset's path delay is its TA plus up to half a sample either way; access bursts likewise about zero
    half = lambda n: rng.uniform(-0.5, 0.5, n) / sps
    air = Air(rng, model, len(g["rach_kind"]), half, half)
    for cls in (lms.TCH, lms.XCCH):
        ta = np.array([ch.handset.ta for ch in model.ch[cls]], np.float32)
        air.delay[cls] = (air.delay[cls] + ta).astype(np.float32)
        air.t[3 + cls] = dev(air.delay[cls])
    buf, cell = radiate_with_noise(ms, air, m["what"], A, F, sps, seed=78)
    grp = setup_group(pkg, ctx, comb, bsic & 7, fn0)
    res = grp.pull(buf.data_ptr(), A * cell, cell, fn0, 0, 8 * F)
    grp.sync()
    rx = pkg.L1Rx(ctx, comb, bsic, band)
    rx.decode(res, fn0)
    got = rx.collect()
    col = grp.collect()
    sent = np.argwhere(m["what"].T != 0)
    assert all(col["valid"][t, a] for t, a in sent), "a clean burst was not detected"
    d = rxm.decode(col, fn0)
    import test_gpu_l1rx
    test_gpu_l1rx.assert_same(got, d, "closed loop")
    # every payload back: TCH stream block b carries encoded block b - 1
    n_tch = 0
    for s in range(len(model.ch[lms.TCH])):
        for b in range(1, g["tch_kind"].shape[1]):
            kind, pl = g["tch_kind"][s, b - 1], g["tch_payload"][s, b - 1]
            if kind == pkg.TCH_SPEECH:
                assert got["tch_status"][s, b] == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(got["tch"][s, b], pl), (s, b)
            else:
                assert got["tch_status"][s, b] & fsm.FACCH_OK and np.array_equal(got["facch"][s, b], pl[:23]), (s, b)
            n_tch += 1
    heard, n_x = set(), 0
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
                    heard.add(s)
                jb = list(got["xcch_fn"][s]).index((fn0 + w[j + 3][0]) % HYPER)
                assert got["xcch_status"][s, jb] == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(got["xcch"][s, jb], want), (s, b)
                n_x += 1
            b += 1
    heard = sorted(heard)
    assert n_tch > 100 and n_x > 40 and len(heard) >= len(sacch) - 2
    assert np.array_equal(got["ms_power"][heard], r["ms_power"][heard]) and np.array_equal(got["ms_ta"][heard], r["ms_ta"][heard])
    assert len({(p, t) for p, t in zip(r["ms_power"][heard], r["ms_ta"][heard])}) > 3
    walk = model.walk(model.ch[lms.RACH][0].m, fn0, F)
    sent_r = [(fn0 + k, g["rach_ra"][j], g["rach_bsic"][j]) for j, (k, _) in enumerate(walk) if g["rach_kind"][j] == 1]
    rr = got["rach"]
    assert list(rr["fn"]) == [u % HYPER for u, _, _ in sent_r] and (rr["arfcn"] == 0).all()
    for (u, ra, b), ok, v in zip(sent_r, rr["ok"], rr["ra"]):
        assert ok == (b == bsic) and v == (ra if b == bsic else 0), u
    assert rr["ok"].any() and not rr["ok"].all()
    ms.destroy(); rx.destroy(); grp.close(); ctx.close()


def test_orders_round_trip(pkg):
    """Three rounds of 104 frames of L1Tx.encode(sibling = rx) -> L1Ms.encode(sibling = tx) -> radiate -> pull ->
    L1Rx.decode.  After each round the decoder's SACCH power / TA on every channel are what the downlink's orders decode to -- the
    orders of the round in which the last SACCH block it heard whole began (a block that straddles two rounds carries the
    header of the round it began in) -- and the handsets are exactly this round's.  No convergence is asserted."""
    import torch
    sps, A, F, bsic, band = 4, 2, 104, 13, 900
    fn0 = 102 * 104 * 3
    rng = np.random.default_rng(99)
    comb = np.array([[1, 1, 7, 0, 1, 0, 0, 0], [1, 7, 0, 0, 0, 1, 0, 0]], np.uint8)
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    tx, rx, ms = pkg.L1Tx(ctx, comb, bsic, band), pkg.L1Rx(ctx, comb, bsic, band), pkg.L1Ms(ctx, comb, bsic, band)
    model = lms.MsModel(comb, bsic, band, oracle=object())  # plan and walk only
    X = model.ch[lms.XCCH]
    sacch = [i for i, c in enumerate(X) if c.sacch]
    # loud and quiet handsets (RSSI either side of the target), some paths longer than their TA
    air = Air(rng, model, 0, lambda n: rng.uniform(-0.4, 1.2, n), lambda n: np.zeros(n), mag=(150.0, 6000.0),
              amp_of_power=10.0 ** ((np.arange(41) - 39) / 20.0))
    for cls in (lms.TCH, lms.XCCH):                          # one path per handset
        for i, ch in enumerate(model.ch[cls]):
            hs = X.index(ch.handset)
            air.gain[cls][i], air.delay[cls][i] = air.gain[lms.XCCH][hs], air.delay[lms.XCCH][hs]
    air.t = [dev(g.view(np.float32).reshape(-1, 2)) for g in air.gain] + [dev(d) for d in air.delay] + [dev(air.amp)]
    grp = setup_group(pkg, ctx, comb, bsic & 7, fn0)
    init = (lms.level_power(band, 40), 0)
    content = lms.Content(rng, p_none=0.0, speech=True)
    last_whole = {}                                          # SACCH channel -> the orders its last whole block carried
    moved = False
    for rnd in range(3):
        fn = fn0 + rnd * F
        nbt, nbx, _ = tx.grid(fn, F)
        dk = dev(np.ones((tx.channels(pkg.L1_XCCH), nbx), np.uint8))
        dp = dev(rng.integers(0, 256, (tx.channels(pkg.L1_XCCH), nbx, 23)).astype(np.uint8))
        tk = dev(np.zeros((tx.channels(pkg.L1_TCH), nbt), np.uint8))
        tp = dev(np.zeros((tx.channels(pkg.L1_TCH), nbt, 33), np.uint8))
        tx.encode(fn, F, tk, tp, dk, dp, None, None, sibling=rx)
        o = tx.collect(state=False)
        want = [(lms.level_power(band, int(o["ms_power"][i])), int(np.float32(o["ms_ta"][i] + np.float32(0.5)))) if i in sacch
                else (-1, -1) for i in range(len(X))]
        g = lms.grids(model, content, fn, F)
        r = gpu_call(ms, fn, F, g, sibling=tx, state=False)
        assert [(int(p), int(t)) for p, t in zip(r["ms_power"], r["ms_ta"])] == want, rnd
        moved |= any(want[i] != init for i in sacch)
        buf, cell = radiate_with_noise(ms, air, r["what"], A, F, sps, seed=rnd)
        res = grp.pull(buf.data_ptr(), A * cell, cell, fn, 0, 8 * F)
        grp.sync()
        rx.decode(res, fn)
        got = rx.collect(state=False)
        # the blocks that closed in this round: begun in it (this round's orders) or in the one before (that round's)
        for i in sacch:
            w = model.walk(X[i].m, fn - F, 2 * F)
            for j, (k, B) in enumerate(w):
                if B == 0 and j + 3 < len(w) and F <= w[j + 3][0] < 2 * F and (k >= F or rnd > 0):
                    b = list(got["xcch_fn"][i]).index((fn - F + w[j + 3][0]) % HYPER)
                    if got["xcch_status"][i, b] & fsm.TCH_GOOD:
                        last_whole[i] = want[i] if k >= F else before[i]
        for i, v in last_whole.items():
            assert (int(got["ms_power"][i]), int(got["ms_ta"][i])) == v, (rnd, i)
        assert len(last_whole) >= len(sacch) // 2, (rnd, len(last_whole))
        before = want
    assert moved and len(last_whole) == len(sacch)
    tx.destroy(); rx.destroy(); ms.destroy(); grp.close(); ctx.close()


# ---- 7 ----
def test_bad_inputs(pkg, ctx):
    """Each returns TRXSIG_EINVAL with nothing launched (the object's last outputs stay as they were)."""
    import torch
    L = ctx.L
    comb = np.array([[5, 1, 7, 1, 0, 0, 0, 0]], np.uint8)
    for bad in (np.array([[4, 0, 0, 0, 0, 0, 0, 0]], np.uint8), np.array([[0, 5, 0, 0, 0, 0, 0, 0]], np.uint8)):
        with pytest.raises(pkg.TrxSigError):
            pkg.L1Ms(ctx, bad, 1)
    with pytest.raises(pkg.TrxSigError):
        pkg.L1Ms(ctx, comb, 64)
    with pytest.raises(pkg.TrxSigError):
        pkg.L1Ms(ctx, comb, 1, band=1234)
    ms = pkg.L1Ms(ctx, comb, 1)
    z = dev(np.zeros((64, 64, 33), np.uint8))
    full = dict(tch_kind=z, tch_payload=z, xcch_kind=z, xcch_payload=z, rach_kind=z, rach_ra=z)
    buf = torch.zeros(8, 1, 640, 2, device="cuda")
    air = dict(tch_gain=buf, tch_delay=buf, xcch_gain=buf, xcch_delay=buf, rach_gain=buf, rach_delay=buf, amp_of_power=buf)
    with pytest.raises(pkg.TrxSigError):
        ms.radiate(buf, 640, 640, **air)                     # before any encode
    for fn, F in ((-1, 1), (HYPER, 1), (0, 0), (0, -5), (0, 1 << 30)):
        with pytest.raises(pkg.TrxSigError):
            ms.encode(fn, F, **full)
    for k in ("tch_kind", "xcch_payload", "rach_ra"):
        with pytest.raises(pkg.TrxSigError):
            ms.encode(4, 1, **{**full, k: None})             # FN 4 is a RACH frame
    other = pkg.L1Tx(ctx, np.array([[5, 1, 7, 0, 0, 0, 0, 0]], np.uint8), 1)
    with pytest.raises(pkg.TrxSigError):
        ms.encode(0, 1, sibling=other, **full)               # a sibling with another plan
    for cls, chan in ((pkg.L1_RACH, 0), (pkg.L1_TCH, 5), (pkg.L1_XCCH, -1), (3, 0)):
        assert L.trxsig_l1ms_open(ms.h, cls, chan) == EINVAL and L.trxsig_l1ms_close(ms.h, cls, chan) == EINVAL
    sdcch = next(i for i in range(ms.channels(1)) if ms.channel(1, i)[2] == pkg.L1_SDCCH4)
    sacch = next(i for i in range(ms.channels(1)) if ms.channel(1, i)[2] == pkg.L1_SACCH_C4)
    for chan, p, t in ((sdcch, 10, 3), (sacch, -1, 3), (sacch, 41, 3), (sacch, 10, -1), (sacch, 10, 64), (10 ** 6, 10, 3)):
        assert L.trxsig_l1ms_set_phy(ms.h, chan, p, t) == EINVAL, (chan, p, t)
    assert L.trxsig_l1ms_set_phy(ms.h, sacch, 0, 63) == 0 and L.trxsig_l1ms_set_phy(ms.h, sacch, 40, 0) == 0
    assert ms.grid(0, 51)[0] == 12 and ms.grid(0, 51)[2] == 27 and L.trxsig_l1ms_channels(ms.h, 3) == EINVAL
    ms.encode(0, 1, **full)                                  # and a good call still goes through
    good = ms.collect()
    for bad in (dict(tch_gain=None), dict(xcch_delay=None), dict(amp_of_power=None)):
        with pytest.raises(pkg.TrxSigError):
            ms.radiate(buf, 640, 640, **{**air, **bad})
    with pytest.raises(pkg.TrxSigError):
        ms.radiate(buf, 100, 640, **air)                     # cells would overlap
    with pytest.raises(pkg.TrxSigError):
        ms.radiate(None, 640, 640, **air)
    ms.radiate(buf, 640, 640, **air)
    again = ms.collect()
    assert all(np.array_equal(good[k], again[k]) for k in KEYS)
    ms.destroy(); other.destroy()


# ---- 8 ----
def test_past_one_launch_slice(pkg):
    """One ARFCN, 8,200 frames = 65,600 slot rows (past a dispatch's 65,535 and past one round of k_l1ms_radiate's workgroups),
    sps 1: encode and radiate equal the same frames in ten calls."""
    import torch
    c = pkg.TrxSig(1, 0)
    c.use_torch_stream()
    comb = np.zeros((1, 8), np.uint8)
    comb[0, 0] = 1
    rng = np.random.default_rng(8)
    fn0, F, cell = 1000, 8200, 157
    model = lms.MsModel(comb, 4, oracle=object())
    content = lms.Content(rng)
    air = Air(rng, model, 0, lambda n: rng.uniform(-2, 2, n), lambda n: np.zeros(n), amp_of_power=np.linspace(0.5, 2.5, 41))
    whole, parts = pkg.L1Ms(c, comb, 4), pkg.L1Ms(c, comb, 4)
    for o in (whole, parts):
        o.set_phy(0, 21, 9)
    ww = gpu_call(whole, fn0, F, lms.grids(model, content, fn0, F))
    bw = torch.full((8 * F, 1, cell, 2), 3.0, device="cuda")
    whole.radiate(bw, cell, cell, **air.kwargs())
    assert 8 * F > 65535 and (ww["what"] != 0).sum() > 7000
    bp = torch.full((8 * F, 1, cell, 2), 3.0, device="cuda")
    step = F // 10
    for p in range(10):
        r = gpu_call(parts, fn0 + p * step, step, lms.grids(model, content, fn0 + p * step, step))
        sl = slice(8 * p * step, 8 * (p + 1) * step)
        assert np.array_equal(r["what"][0], ww["what"][0, sl]) and np.array_equal(r["bits"][0], ww["bits"][0, sl]), p
        parts.radiate(bp[sl], cell, cell, **air.kwargs())
    for k in KEYS[2:]:
        assert np.array_equal(r[k], ww[k]), k
    torch.cuda.synchronize()
    assert torch.equal(bw.view(torch.int32), bp.view(torch.int32))
    last = int(np.flatnonzero(ww["what"][0])[-1])
    assert last > 65535 and last % 8 == 0 and float(bw[last].abs().max()) > 0.1           # the last burst was radiated
    nxt = bw[last + 1, 0].cpu().numpy()                      # TN 1: 156 zeros, then the buffer as it was
    assert not nxt[:156].any() and (nxt[156] == 3.0).all()
    whole.destroy(); parts.destroy(); c.close()
