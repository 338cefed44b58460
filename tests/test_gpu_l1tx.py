"""GPU parity of the downlink L1 multiplexer (trxsig_l1tx.h) against its literal CPU model (tests/l1_mux_model.py): random plans
and grids with every TCH kind, missing XCCH / CCCH frames, closed channels and idle fill; random splits of one span; spans
across the 5304-frame period and the hyperframe wrap; SACCH orders from an L1Rx sibling; datagrams through a Transceiver
group's transmit queue; the production plan; the bad-input rules.  Byte-exact in d_bits, d_what, the orders and the state."""
import ctypes as C

import numpy as np
import pytest

import _pkg
import l1_demux_model as ldm
import l1_mux_model as lmm

pytestmark = pytest.mark.gpu
HYPER = lmm.HYPERFRAME


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


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_plan(rng, A, c5=True):
    comb = rng.choice(np.array([0, 1, 1, 7], np.uint8), (A, 8))
    if c5:
        comb[0, 0] = 5
    return comb


class Content:
    """Payloads keyed by (class, channel, the block's first frame, unwrapped), so that any split of a span asks for the same."""

    def __init__(self, rng, p_none=0.25):
        self.rng, self.p_none, self.d = rng, p_none, {}

    def get(self, cls, i, u):
        key = (cls, i, u)
        if key not in self.d:
            r = self.rng
            if cls == lmm.TCH:
                kind = int(r.choice([0, 1, 1, 2, 3], p=[0.2, 0.35, 0.2, 0.2, 0.05]))
                self.d[key] = (kind, r.integers(0, 256, 33).astype(np.uint8))
            else:
                kind = 0 if r.random() < self.p_none else 1
                self.d[key] = (kind, r.integers(0, 256, 23).astype(np.uint8))
        return self.d[key]


def grids(model, content, fn, F):
    """The call's grids, [n][nb] and [n][nb][33 / 23], from the model's walk of each channel."""
    out = {}
    nb = dict(zip((lmm.TCH, lmm.XCCH, lmm.CCCH), model.grid(fn, F)))
    for cls, width in ((lmm.TCH, 33), (lmm.XCCH, 23), (lmm.CCCH, 23)):
        chans = model.ch[cls]
        kind = np.zeros((len(chans), nb[cls]), np.uint8)
        pay = np.zeros((len(chans), nb[cls], width), np.uint8)
        for i, c in enumerate(chans):
            b = 0
            for k, B in model.walk(c.m, fn, F):
                if B == 0:
                    kind[i, b], pay[i, b] = content.get(cls, i, fn + k)
                    b += 1
        out[cls] = (kind, pay)
    return out, nb


def gpu_call(pkg, l1, fn, F, g, sibling=None):
    t = {k: (dev(v[0]), dev(v[1])) for k, v in g.items()}
    l1.encode(fn, F, t[lmm.TCH][0], t[lmm.TCH][1], t[lmm.XCCH][0], t[lmm.XCCH][1], t[lmm.CCCH][0], t[lmm.CCCH][1], sibling=sibling)
    r = l1.collect()
    r["_keep"] = t
    return r


def model_call(model, fn, F, g, sib=None):
    return model.encode(fn, F, g[lmm.TCH][0], g[lmm.TCH][1], g[lmm.XCCH][0], g[lmm.XCCH][1], g[lmm.CCCH][0], g[lmm.CCCH][1],
                        sib=sib)


def assert_same(r, m, what=""):
    assert np.array_equal(r["what"], m["what"]), (what, np.argwhere(r["what"] != m["what"])[:8])
    bad = np.argwhere((r["bits"] != m["bits"]).any(-1))
    assert len(bad) == 0, (what, bad[:8], r["what"][tuple(bad[0])] if len(bad) else None)
    assert np.array_equal(r["ms_power"], m["ms_power"]), what
    assert np.array_equal(r["ms_ta"].view(np.uint32), m["ms_ta"].view(np.uint32)), what


def si_frames(rng):
    return rng.integers(0, 256, (4, 23)).astype(np.uint8)


@pytest.mark.parametrize("seed", range(4))
def test_random_plans_against_the_model(pkg, ctx, oracle, seed):
    """Random plans (1-8 ARFCNs), random grids, contiguous calls of random lengths with open / close between them."""
    rng = np.random.default_rng(100 + seed)
    A = int(rng.integers(1, 9))
    comb = random_plan(rng, A, c5=seed != 3)
    bsic = int(rng.integers(0, 64))
    l1 = pkg.L1Tx(ctx, comb, bsic)
    model = lmm.MuxModel(comb, bsic, oracle=oracle)
    if seed % 2 == 0:
        si = si_frames(rng)
        l1.set_si(si); model.set_si(si)
    content = Content(rng)
    fn = int(rng.integers(0, HYPER - 2000))
    seen = set()
    for call in range(6):
        F = int(rng.choice([1, 3, 26, 51, 60, 104]))
        for _ in range(3):                                   # open / close between calls
            cls = int(rng.choice([pkg.L1_TCH, pkg.L1_XCCH, pkg.L1_CCCH]))
            n = l1.channels(cls)
            if n:
                i = int(rng.integers(0, n))
                mcls = lmm.CCCH if cls == pkg.L1_CCCH else cls
                if rng.random() < 0.5:
                    l1.close(cls, i); model.close(mcls, i)
                else:
                    l1.open(cls, i); model.open(mcls, i)
        g, nb = grids(model, content, fn, F)
        assert l1.grid(fn, F) == (nb[lmm.TCH], nb[lmm.XCCH], nb[lmm.CCCH])
        r = gpu_call(pkg, l1, fn, F, g)
        m = model_call(model, fn, F, g)
        assert_same(r, m, (seed, call, fn, F))
        seen |= set(np.unique(r["what"]).tolist())
        fn += F
    assert {lmm.W_TCH, lmm.W_XCCH} <= seen or A == 1, seen   # the test reached the traffic paths
    if seed % 2 == 0 and seed != 3:
        assert {lmm.W_FCCH, lmm.W_SCH, lmm.W_BCCH, lmm.W_CCCH} <= seen, seen
    l1.destroy()


def test_idle_fill_after_close(pkg, ctx, oracle):
    """close queues numFrames dummy bursts after the pending block; a second call finishes them; open cancels the rest."""
    comb = np.array([[5, 1, 7, 0, 0, 0, 0, 0]], np.uint8)
    l1 = pkg.L1Tx(ctx, comb, 5)
    model = lmm.MuxModel(comb, 5, oracle=oracle)
    content = Content(np.random.default_rng(7), p_none=0.0)
    fn = 1000
    counts = 0
    for call, F in enumerate([30, 7, 13, 40, 9, 60]):
        if call == 1:
            for cls in (pkg.L1_TCH, pkg.L1_XCCH, pkg.L1_CCCH):
                for i in range(l1.channels(cls)):
                    l1.close(cls, i); model.close(lmm.CCCH if cls == pkg.L1_CCCH else cls, i)
        if call == 4:
            l1.open(pkg.L1_XCCH, 3); model.open(lmm.XCCH, 3)
        g, _ = grids(model, content, fn, F)
        r = gpu_call(pkg, l1, fn, F, g)
        m = model_call(model, fn, F, g)
        assert_same(r, m, (call, fn, F))
        counts += int((r["what"] == lmm.W_IDLE).sum())
        fn += F
    assert counts > 24, counts                               # idle fill was reached
    l1.destroy()


def split_vs_whole(pkg, ctx, oracle, rng, comb, fn0, F, cuts, sib=False):
    bsic = int(rng.integers(0, 64))
    si = si_frames(rng)
    content = Content(rng)
    objs = []
    for _ in range(2):
        l1 = pkg.L1Tx(ctx, comb, bsic)
        l1.set_si(si)
        objs.append(l1)
    model = lmm.MuxModel(comb, bsic, oracle=oracle)
    model.set_si(si)
    g, _ = grids(model, content, fn0, F)
    whole = gpu_call(pkg, objs[0], fn0 % HYPER, F, g)
    assert_same(whole, model_call(model, fn0, F, g), "whole")
    st_whole = [whole[k] for k in ("tch_state", "xcch_state", "ccch_state")]
    edges = [0] + sorted(cuts) + [F]
    parts = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        if hi == lo:
            continue
        gp, _ = grids(model, content, fn0 + lo, hi - lo)
        parts.append(gpu_call(pkg, objs[1], (fn0 + lo) % HYPER, hi - lo, gp))
    bits = np.concatenate([p["bits"] for p in parts], axis=1)
    what = np.concatenate([p["what"] for p in parts], axis=1)
    assert np.array_equal(what, whole["what"])
    assert np.array_equal(bits, whole["bits"])
    for a, b in zip(st_whole, [parts[-1][k] for k in ("tch_state", "xcch_state", "ccch_state")]):
        assert np.array_equal(a, b)
    for l1 in objs:
        l1.destroy()
    return whole


@pytest.mark.parametrize("seed", range(3))
def test_random_splits_equal_one_call(pkg, ctx, oracle, seed):
    """One call of F frames against calls split at random frame boundaries, 1-frame calls and cuts inside blocks included."""
    rng = np.random.default_rng(200 + seed)
    comb = random_plan(rng, int(rng.integers(1, 5)))
    F = 104
    cuts = list(rng.choice(np.arange(1, F), size=6, replace=False)) + [1, 2]
    fn0 = int(rng.integers(0, HYPER - F))
    w = split_vs_whole(pkg, ctx, oracle, rng, comb, fn0, F, cuts)
    assert (w["what"] == lmm.W_TCH).any() or (comb != 1).all()


@pytest.mark.parametrize("fn0", [5304 * 7 - 37, HYPER - 61])
def test_spans_across_the_wraps(pkg, ctx, oracle, fn0):
    """Spans across the 5304-frame period and the hyperframe wrap, split and whole, against the model."""
    rng = np.random.default_rng(fn0 % 997)
    comb = random_plan(rng, 3)
    split_vs_whole(pkg, ctx, oracle, rng, comb, fn0, 130, [37, 61, 62, 90])


def uplink_frames(maps_ul, name, fn, F):
    m = maps_ul[name]
    return sum(1 for u in range(fn, fn + F) if m.reverse(u % HYPER) >= 0)


def sibling_pull(pkg, rng, A, F, valid):
    T = 8 * F
    n = T * A
    row = np.arange(n, dtype=np.int32).reshape(T, A)
    t = dict(row=dev(row), valid=dev(np.full(n, pkg.F_DETECT if valid else 0, np.uint8)),
             amp=dev((rng.standard_normal((n, 2)) * 3000).astype(np.float32)),
             toa=dev((rng.standard_normal(n) * 4).astype(np.float32)), soft=dev(rng.random((n, 148)).astype(np.float32)))
    res = pkg.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=n, d_row=t["row"].data_ptr(), d_valid=t["valid"].data_ptr(), d_flags=None,
                             d_amp=t["amp"].data_ptr(), d_toa=t["toa"].data_ptr(), d_avgpwr=None, d_threshold=None,
                             d_soft=t["soft"].data_ptr(), soft_stride=148)
    return res, t


def test_sacch_orders_from_an_l1rx_sibling(pkg, ctx, oracle):
    """An L1Rx sibling decodes pulls with and without bursts on its SACCH channels; each L1Tx call's SACCH headers and orders
    follow the sibling's RSSI / timing / actual power and TA exactly when it accepted a burst since the last decision."""
    rng = np.random.default_rng(11)
    comb = np.array([[5, 1, 7, 1, 0, 0, 0, 0], [1, 1, 0, 7, 0, 0, 0, 0]], np.uint8)
    A = comb.shape[0]
    rx = pkg.L1Rx(ctx, comb, 9)
    tx = pkg.L1Tx(ctx, comb, 9, rssi_target=-15.0)
    model = lmm.MuxModel(comb, 9, oracle=oracle)
    maps_ul = ldm.load_mappings()
    names = []
    for i in range(rx.channels(pkg.L1_XCCH)):
        a, tn, kind, sub = rx.channel(pkg.L1_XCCH, i)
        names.append({pkg.L1_SACCH_TF: "SACCH_TF_T%d" % tn, pkg.L1_SACCH_C8: "SACCH_C8_%dU" % sub,
                      pkg.L1_SACCH_C4: "SACCH_C4_%dU" % sub}.get(kind))
    content = Content(rng, p_none=0.1)
    count = np.zeros(len(names), np.int64)
    fn = 40000
    changed = 0
    for call in range(8):
        F = 104 if call % 3 else 51
        valid = call % 4 != 2
        res, keep = sibling_pull(pkg, rng, A, F, valid)
        rx.decode(res, fn - F)                               # the uplink of the frames before this call
        s = rx.collect(state=False)
        if valid:
            count += np.array([uplink_frames(maps_ul, nm, fn - F, F) if nm else 0 for nm in names])
        sib = dict(rssi=s["xcch_rssi"], timing=s["xcch_timing"], power=s["ms_power"], ta=s["ms_ta"], count=count.copy())
        g, _ = grids(model, content, fn, F)
        before = [(c.power, float(c.ta)) for c in model.ch[lmm.XCCH]]
        r = gpu_call(pkg, tx, fn, F, g, sibling=rx)
        m = model_call(model, fn, F, g, sib=sib)
        assert_same(r, m, (call, fn))
        changed += [(c.power, float(c.ta)) for c in model.ch[lmm.XCCH]] != before
        fn += F
    assert changed >= 2, changed                             # orders moved with the sibling's phy
    other = pkg.L1Rx(ctx, np.array([[5, 1, 7, 1, 0, 0, 0, 0], [1, 1, 0, 1, 0, 0, 0, 0]], np.uint8), 9)
    g, _ = grids(model, content, fn, 1)
    t = {k: (dev(v[0]), dev(v[1])) for k, v in g.items()}
    with pytest.raises(pkg.TrxSigError):
        tx.encode(fn, 1, t[lmm.TCH][0], t[lmm.TCH][1], t[lmm.XCCH][0], t[lmm.XCCH][1], t[lmm.CCCH][0], t[lmm.CCCH][1], sibling=other)
    other.destroy(); rx.destroy(); tx.destroy()


def test_datagrams_through_the_transmit_queue(pkg, ctx, oracle):
    """datagrams -> trxsig_trxgroup_add_bursts -> trxsig_trxgroup_push over the same frames gives the same bits, with
    d_from_queue = 1 exactly where d_what != 0; spans of 32 frames keep every queue under its 256 bursts."""
    import torch
    rng = np.random.default_rng(5)
    comb = np.array([[5, 1, 7, 1, 1, 0, 7, 1], [1, 1, 1, 1, 1, 1, 1, 1], [7, 0, 0, 1, 0, 0, 0, 0]], np.uint8)
    A = comb.shape[0]
    l1 = pkg.L1Tx(ctx, comb, 21)
    model = lmm.MuxModel(comb, 21, oracle=oracle)
    si = si_frames(rng)
    l1.set_si(si); model.set_si(si)
    grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD)
    content = Content(rng)
    fn = 2000
    for call in range(3):
        F = 32
        g, _ = grids(model, content, fn, F)
        r = gpu_call(pkg, l1, fn, F, g)
        assert_same(r, model_call(model, fn, F, g), call)
        dg, ar = l1.datagrams()
        on = r["what"] != 0
        assert len(dg) == int(on.sum())
        # (FN, TN, ARFCN) order and the datagram layout
        key = [(int.from_bytes(bytes(d[1:5]), "big"), int(d[0]), int(a)) for d, a in zip(dg, ar)]
        assert key == sorted(key)
        for d, a in zip(dg[:50], ar[:50]):
            f, tn = int.from_bytes(bytes(d[1:5]), "big"), int(d[0])
            assert d[5] == 0 and np.array_equal(d[6:], r["bits"][a, 8 * (f - fn) + tn])
        with pytest.raises(pkg.TrxSigError):
            l1.datagrams(cap=len(dg) - 1)
        grp.add_bursts(dg, ar)
        for a in range(A):
            assert grp.tx_queue_size(a)[1] is False
        b, _, fq = grp.push(fn, 0, 8 * F)
        torch.cuda.synchronize()
        b, fq = b.cpu().numpy(), fq.cpu().numpy()
        assert np.array_equal(fq != 0, on)
        assert np.array_equal(b[on], r["bits"][on])
        fn += F
    grp.close(); l1.destroy()


def test_production_plan_against_the_model(pkg, ctx, oracle):
    """128 ARFCNs (C0: V on TN 0, VII on TN 1, I elsewhere; I on every other carrier) x 104 frames over two calls, then a
    680-frame call, against the model."""
    comb = np.ones((128, 8), np.uint8)
    comb[0, 0], comb[0, 1] = 5, 7
    rng = np.random.default_rng(3)
    l1 = pkg.L1Tx(ctx, comb, 33)
    model = lmm.MuxModel(comb, 33, oracle=oracle)
    si = si_frames(rng)
    l1.set_si(si); model.set_si(si)
    content = Content(rng)
    fn = 123456
    for F in (104, 104, 680):
        g, nb = grids(model, content, fn, F)
        r = gpu_call(pkg, l1, fn, F, g)
        assert_same(r, model_call(model, fn, F, g), F)
        assert (r["what"] == lmm.W_TCH).sum() > 90000 * F // 104
        fn += F
    l1.destroy()


def test_bad_inputs(pkg, ctx):
    comb = np.array([[5, 1, 7, 1, 0, 0, 0, 0]], np.uint8)
    for bad in (np.array([[4, 0, 0, 0, 0, 0, 0, 0]], np.uint8), np.array([[0, 5, 0, 0, 0, 0, 0, 0]], np.uint8)):
        with pytest.raises(pkg.TrxSigError):
            pkg.L1Tx(ctx, bad, 1)
    with pytest.raises(pkg.TrxSigError):
        pkg.L1Tx(ctx, comb, 64)
    with pytest.raises(pkg.TrxSigError):
        pkg.L1Tx(ctx, comb, 1, band=1234)
    l1 = pkg.L1Tx(ctx, comb, 1)
    z = dev(np.zeros((64, 64, 33), np.uint8))
    full = dict(tch_kind=z, tch_payload=z, xcch_kind=z, xcch_payload=z, ccch_kind=z, ccch_payload=z)
    for fn, F in ((-1, 1), (HYPER, 1), (0, 0), (0, -5)):
        with pytest.raises(pkg.TrxSigError):
            l1.encode(fn, F, **full)
    for k in ("tch_kind", "xcch_payload", "ccch_kind"):
        with pytest.raises(pkg.TrxSigError):
            l1.encode(0, 1, **{**full, k: None})
    with pytest.raises(pkg.TrxSigError):
        l1.encode(0, 1 << 30, **full)                        # output above the bound
    with pytest.raises(pkg.TrxSigError):
        l1.open(pkg.L1_RACH, 0)
    with pytest.raises(pkg.TrxSigError):
        l1.close(pkg.L1_TCH, 5)
    l1.encode(0, 1, **full)                                  # and a good call still goes through
    l1.collect()
    l1.destroy()
    big = pkg.L1Tx(ctx, np.zeros((0xffff, 8), np.uint8), 1)
    with pytest.raises(pkg.TrxSigError):
        big.encode(0, 20000, **full)                         # 0xffff * 8 * 20000 * 148 bytes > 2^34
    big.destroy()


# ---- end to end: push -> GMSK -> a Transceiver group pull -> the stream decoders indexed by the downlink mappings ----
class AirContent(Content):
    """Speech or FACCH on every TCH block (the last 4 payload bits of speech are not coded: zero), frames on most XCCH / CCCH."""

    def get(self, cls, i, u):
        key = (cls, i, u)
        if cls == lmm.TCH and key not in self.d:
            kind = int(self.rng.choice([1, 2], p=[0.7, 0.3]))
            pl = self.rng.integers(0, 256, 33).astype(np.uint8)
            pl[32] &= 0xF0
            self.d[key] = (kind, pl)
        return super().get(cls, i, u)


def full_blocks(c, fn, F, A, tch):
    """The channel's blocks wholly inside [fn, fn + F), from the first burst with B = 0 (TCH: B mod 8 = 0): (first frame, the
    pull rows (8 k + tn) * A + a of its bursts in time order)"""
    w = lmm.MuxModel.walk(c.m, fn, F)
    period = 8 if tch else 4
    s = next((j for j, (k, _) in enumerate(w) if c.m.reverse(fn + k) % period == 0), len(w))
    w = w[s:]
    return [(fn + w[j][0], [(8 * k + c.tn) * A + c.a for k, _ in w[j:j + 4]]) for j in range(0, len(w) - 3, 4)]


def test_loop_over_the_air(pkg, oracle):
    """L1Tx calls of 32 frames -> datagrams -> trxsig_trxgroup_add_bursts / _push -> GMSK ->
    trxsig_trxgroup_pull (every slot a traffic slot) -> trxsig_fec_xcch_decode_stream / trxsig_fec_tch_decode_stream indexed by
    the downlink mappings.  Every SDCCH / SACCH / CCCH / BCCH frame and every speech and FACCH block whose bursts lie in the window
    comes back; SACCH octets 0..1 are the model's header, with orders taken from an L1Rx sibling."""
    import torch
    import fec_stream_model as fsm
    sps, A, F, fn0, bsic, band = 4, 2, 224, 2652, 21, 900   # fn0 = 102 * 26: on the 26-, 51- and 102-frame grids
    tsc = bsic & 7
    comb = np.array([[5, 1, 7, 1, 0, 0, 0, 0], [1, 7, 0, 1, 1, 0, 0, 0]], np.uint8)
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(31)
    tx = pkg.L1Tx(ctx, comb, bsic, band)
    rx = pkg.L1Rx(ctx, comb, bsic, band)
    model = lmm.MuxModel(comb, bsic, band=band, oracle=oracle)
    si = si_frames(rng)
    tx.set_si(si); model.set_si(si)
    # the sibling decodes an uplink with a burst on every slot: the first SACCH block of each channel takes its orders from it
    maps_ul = ldm.load_mappings()
    names = []
    for i in range(rx.channels(pkg.L1_XCCH)):
        _, tn, kind, sub = rx.channel(pkg.L1_XCCH, i)
        names.append({pkg.L1_SACCH_TF: "SACCH_TF_T%d" % tn, pkg.L1_SACCH_C8: "SACCH_C8_%dU" % sub,
                      pkg.L1_SACCH_C4: "SACCH_C4_%dU" % sub}.get(kind))
    res_ul, keep_ul = sibling_pull(pkg, rng, A, 104, True)
    rx.decode(res_ul, fn0 - 104)
    s = rx.collect(state=False)
    count = np.array([uplink_frames(maps_ul, nm, fn0 - 104, 104) if nm else 0 for nm in names])
    sib = dict(rssi=s["xcch_rssi"], timing=s["xcch_timing"], power=s["ms_power"], ta=s["ms_ta"], count=count)
    content = AirContent(rng, p_none=0.1)
    grp_tx = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD)
    T = 8 * F
    pushed = np.zeros((A, T, 148), np.uint8)
    from_q = np.zeros((A, T), np.uint8)
    what = np.zeros((A, T), np.uint8)
    for c0 in range(0, F, 32):                               # 32 frames: at most 256 bursts per ARFCN queue
        g, _ = grids(model, content, fn0 + c0, 32)
        r = gpu_call(pkg, tx, fn0 + c0, 32, g, sibling=rx)
        assert_same(r, model_call(model, fn0 + c0, 32, g, sib=sib), c0)
        dg, ar = tx.datagrams()
        grp_tx.add_bursts(dg, ar)
        b, _, fq = grp_tx.push(fn0 + c0, 0, 256)
        torch.cuda.synchronize()
        pushed[:, 8 * c0:8 * c0 + 256] = b.cpu().numpy()
        from_q[:, 8 * c0:8 * c0 + 256] = fq.cpu().numpy()
        what[:, 8 * c0:8 * c0 + 256] = r["what"]
    assert np.array_equal(from_q != 0, what != 0)
    # GMSK (synth.bursts_from_bits: the burst placement the receive tests use): the normal bursts that came out of the queue
    # (FCCH / SCH are not normal bursts), each in its slot's cell
    from openbts_ttsou_amd import synth
    sent = [(t, a) for t in range(T) for a in range(A) if from_q[a, t] and what[a, t] not in (lmm.W_FCCH, lmm.W_SCH)]
    xs, offs, lens, _ = synth.bursts_from_bits(np.stack([pushed[a, t] for t, a in sent]), sps, seed=32, sigmas=(0.0, 0.02),
                                               max_delay=0.5)
    cell = 160 * sps
    x = np.zeros((T, A, cell), np.complex64)
    for i, (t, a) in enumerate(sent):
        nsmp = (156 + (t % 8 % 4 == 0)) * sps
        v = xs[offs[i]:offs[i] + lens[i]][:nsmp]
        x[t, a, :len(v)] = v
    grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn0, 0))
    for a in range(A):
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % tsc] + \
                   ["CMD SETSLOT %d 1" % tn for tn in range(8)] + ["CMD POWERON"]:
            grp.control(a, cmd)
    dx = torch.from_numpy(x.view(np.float32).reshape(-1)).to("cuda:0")
    grp.pull(dx.data_ptr(), A * cell, cell, fn0, 0, T)
    grp.sync()
    col = grp.collect()
    assert all(col["valid"][t, a] for t, a in sent), "a clean burst was not detected"
    rows = dev(col["soft"].reshape(T * A, 148).astype(np.float32))
    ok = fsm.DECODED | fsm.TCH_GOOD
    # XCCH-like channels: SDCCH / SACCH, CCCH, BCCH
    checked = {"sdcch": 0, "sacch": 0, "ccch": 0, "bcch": 0}
    for cls in (lmm.XCCH, lmm.CCCH, lmm.BCCH):
        chans = model.ch[cls]
        blocks = [full_blocks(c, fn0, F, A, False) for c in chans]
        nb = max(len(bl) for bl in blocks)
        idx = np.full((len(chans), 4 * nb), -1, np.int32)
        for i, bl in enumerate(blocks):
            for j, (_, rr) in enumerate(bl):
                idx[i, 4 * j:4 * j + 4] = rr
        st = torch.zeros(len(chans), pkg.XCCH_RX_STATE_BYTES, dtype=torch.uint8, device="cuda")
        status = torch.zeros(len(chans), nb, dtype=torch.uint8, device="cuda")
        frames = torch.zeros(len(chans), nb, 23, dtype=torch.uint8, device="cuda")
        ctx.fec_xcch_decode_stream(rows, dev(idx), st, status, frames)
        torch.cuda.synchronize()
        status, frames = status.cpu().numpy(), frames.cpu().numpy()
        for i, (c, bl) in enumerate(zip(chans, blocks)):
            for j, (u, _) in enumerate(bl):
                if cls == lmm.BCCH:
                    want, key = si[lmm.SI_OF_TC[((u % HYPER) // 51) % 8]], "bcch"
                else:
                    kind, pay = content.get(cls, i, u)
                    if kind != 1:
                        continue
                    want, key = pay, "ccch" if cls == lmm.CCCH else "sdcch"
                    if c.sacch:
                        want, key = model.sacch_frame(pay, c.power, c.ta), "sacch"
                        assert tuple(frames[i, j, :2]) == lmm.sacch_header(band, c.power, c.ta), (i, u)
                assert status[i, j] == ok and np.array_equal(frames[i, j], want), (cls, i, u)
                checked[key] += 1
    assert checked["sdcch"] >= 20 and checked["sacch"] >= 8 and checked["ccch"] >= 4 and checked["bcch"] >= 2, checked
    assert any((c.power, float(c.ta)) != (40, 0.0) for c in model.ch[lmm.XCCH] if c.sacch)   # the orders moved
    # TCH: stream block b (b >= 1) is encoder block b - 1
    chans = model.ch[lmm.TCH]
    blocks = [full_blocks(c, fn0, F, A, True) for c in chans]
    nb = max(len(bl) for bl in blocks)
    idx = np.full((len(chans), 4 * nb), -1, np.int32)
    for i, bl in enumerate(blocks):
        for j, (_, rr) in enumerate(bl):
            idx[i, 4 * j:4 * j + 4] = rr
    st = torch.zeros(len(chans), pkg.TCH_RX_STATE_BYTES, dtype=torch.uint8, device="cuda")
    status = torch.zeros(len(chans), nb, dtype=torch.uint8, device="cuda")
    o33 = torch.zeros(len(chans), nb, 33, dtype=torch.uint8, device="cuda")
    o23 = torch.zeros(len(chans), nb, 23, dtype=torch.uint8, device="cuda")
    ctx.fec_tch_decode_stream(rows, dev(idx), st, status, o33, o23, b0=dev(np.zeros(len(chans), np.uint8)))
    torch.cuda.synchronize()
    status, o33, o23 = status.cpu().numpy(), o33.cpu().numpy(), o23.cpu().numpy()
    n_speech = n_facch = 0
    for i, bl in enumerate(blocks):
        for b in range(1, len(bl)):
            kind, pay = content.get(lmm.TCH, i, bl[b - 1][0])
            if kind == pkg.TCH_SPEECH:
                assert status[i, b] & fsm.TCH_GOOD and np.array_equal(o33[i, b], pay), (i, b)
                n_speech += 1
            else:
                assert status[i, b] & fsm.FACCH_OK and np.array_equal(o23[i, b], pay[:23]), (i, b)
                n_facch += 1
    assert n_speech >= 100 and n_facch >= 30, (n_speech, n_facch)
    tx.destroy(); rx.destroy(); grp.close(); grp_tx.close(); ctx.close()


def test_launches_past_one_slice(pkg, ctx):
    """A call whose TCH grid passes a dispatch's 65535 block rows (k_l1tx_encode in two slices) equals ten calls under it, and
    the datagrams of a call of more than 65535 slot rows (the compaction in two slices) are every non-empty slot in order."""
    import torch
    comb = np.zeros((1, 8), np.uint8)
    comb[0, 0] = 1
    rng = np.random.default_rng(8)
    fn0, F = 1000, 290000
    model = lmm.MuxModel(comb, 4, oracle=object())
    content = Content(rng)
    g, nb = grids(model, content, fn0, F)
    assert nb[lmm.TCH] > 65535
    whole = pkg.L1Tx(ctx, comb, 4)
    ww = gpu_call(pkg, whole, fn0, F, g)
    parts = pkg.L1Tx(ctx, comb, 4)
    step = F // 10
    for p in range(10):
        gp, _ = grids(model, content, fn0 + p * step, step)
        r = gpu_call(pkg, parts, fn0 + p * step, step, gp)
        sl = slice(8 * p * step, 8 * (p + 1) * step)
        assert np.array_equal(r["what"][0], ww["what"][0, sl]), p
        assert np.array_equal(r["bits"][0], ww["bits"][0, sl]), p
    for k in ("tch_state", "xcch_state"):
        assert np.array_equal(r[k], ww[k])
    assert (ww["what"] == lmm.W_TCH).sum() > 4 * 65535               # the bursts of more than 65535 blocks
    whole.destroy(); parts.destroy()
    del ww, r
    l1 = pkg.L1Tx(ctx, comb, 4)
    F = 8200                                                 # 65,600 slot rows
    g, _ = grids(model, content, fn0, F)
    r = gpu_call(pkg, l1, fn0, F, g)
    dg, ar = l1.datagrams()
    on = np.argwhere(r["what"][0] != 0)[:, 0]
    assert len(dg) == len(on) and (ar == 0).all() and on[-1] >= 65535
    fn_of = np.array([int.from_bytes(bytes(d[1:5]), "big") for d in dg])
    assert np.array_equal(8 * (fn_of - fn0) + dg[:, 0], on)
    assert np.array_equal(dg[:, 6:], r["bits"][0, on])
    l1.destroy()
