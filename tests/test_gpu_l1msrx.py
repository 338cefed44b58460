"""GPU parity of the mobile-side downlink L1 (trxsig_l1msrx.h) against its literal model (tests/l1_msrx_model.py): every output
array and the decoders' state bytes exactly, FER as bit patterns.  Random plans and streams (missing and invalid bursts, both
wire settings, closed channels), chaining across the 5304 period and the hyperframe wrap, lists past one wave and one finish
block, the SCH verdicts, the bad-input rules, the closed loops L1Tx -> bits -> L1MsRx and L1Tx -> GMSK -> TrxGroup.pull ->
L1MsRx, and L1Ms.follow against set_phy with the decoded orders."""
import ctypes as C

import numpy as np
import pytest

import _pkg
import fec_stream_model as fsm
import l1_demux_model as ldm
import l1_msrx_model as lrm
import l1_mux_model as lmm
import test_l1_msrx_model as tm

pytestmark = pytest.mark.gpu
HYPER = lrm.HYPERFRAME
EINVAL = -1
BLOCK_KEYS = ("tch", "xcch", "ccch", "bcch")


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
def prims():
    return fsm.Prims()


@pytest.fixture(scope="module")
def tx():
    import fectxbind
    return fectxbind.FecTxOracle()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Feed:
    """A trxsig_trxgroup_result built from tensors -- slot (t, a) present where `present`, its 148 soft values in a row of
    `stride` floats, rows in random order among spare ones, a fraction of the rows not valid -- and what trxsig_trxgroup_collect
    would report for it (the model's input)."""

    def __init__(self, pkg, rng, soft, present, p_invalid=0.1, stride=160, sps=4):
        self.pkg = pkg
        T, A = present.shape
        n = int(present.sum())
        n_rows = n + 5
        row = np.full((T, A), -1, np.int32)
        row[present] = rng.permutation(n_rows)[:n]
        rows = rng.random((n_rows, stride)).astype(np.float32)
        rows[row[present], :148] = soft[present]
        valid = (rng.random(n_rows) >= p_invalid).astype(np.uint8) * pkg.F_DETECT
        amp = (rng.standard_normal((n_rows, 2)) * 3000).astype(np.float32)
        toa = (rng.standard_normal(n_rows) * 3).astype(np.float32)
        self.T, self.A, self.n_rows, self.stride = T, A, n_rows, stride
        self.t = dict(row=dev(row), valid=dev(valid), amp=dev(amp), toa=dev(toa), soft=dev(rows))
        self.res = self.result(0, T // 8)
        ok = (row >= 0) & (valid[np.maximum(row, 0)] != 0)
        r = np.maximum(row, 0)
        a = amp[r]
        n2 = (a[..., 1] * a[..., 1] + a[..., 0] * a[..., 0]).astype(np.float32)
        absA = np.sqrt(n2.astype(np.float64)).astype(np.float32)
        rssi = np.floor(20.0 * np.log10(9450.0 / absA.astype(np.float64))).astype(np.int64)
        x = toa[r].astype(np.float64) * 256.0 / sps
        timing = (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)
        self.col = dict(valid=ok, soft=rows[r, :148], rssi=np.where(ok, rssi, 0), timing=np.where(ok, timing, 0))

    def result(self, lo, hi):
        """the result of frames [lo, hi)"""
        t = self.t
        part = t["row"][8 * lo:8 * hi].contiguous()
        self.t["part_%d_%d" % (lo, hi)] = part
        return self.pkg.TrxGroupResult(n_slots=8 * (hi - lo), n_arfcn=self.A, n_rows=self.n_rows, d_row=part.data_ptr(),
                                       d_valid=t["valid"].data_ptr(), d_flags=None, d_amp=t["amp"].data_ptr(),
                                       d_toa=t["toa"].data_ptr(), d_avgpwr=None, d_threshold=None, d_soft=t["soft"].data_ptr(),
                                       soft_stride=self.stride)


def as_model(g):
    """L1MsRx.collect() in the model's layout"""
    out = {}
    for key in BLOCK_KEYS:
        out[key] = dict(status=g[key + "_status"], frames=g[key], fer=g[key + "_fer"], fn=g[key + "_fn"], state=g.get(key + "_state"),
                        rssi=g[key + "_rssi"], timing=g[key + "_timing"],
                        facch=g["facch"] if key == "tch" else np.zeros(g[key].shape[:2] + (23,), np.uint8),
                        tc=g["bcch_tc"] if key == "bcch" else np.zeros(g[key].shape[:2], np.int32))
    out["xcch"]["power"], out["xcch"]["ta"] = g["ord_power"], g["ord_ta"]
    out["sch"], out["fcch"] = g["sch"], g["fcch"]
    return out


def assert_same(g, m, what=""):
    """g: as_model(L1MsRx.collect()), m: the model's output"""
    for key in BLOCK_KEYS:
        go, mo = g[key], m[key]
        for k in ("status", "fn", "rssi", "timing", "frames", "facch", "tc", "state"):
            assert go[k].shape == mo[k].shape and np.array_equal(go[k], mo[k]), (what, key, k, np.argwhere(go[k] != mo[k])[:5]
                                                                                    if go[k].shape == mo[k].shape else (go[k].shape, mo[k].shape))
        assert np.array_equal(go["fer"].view(np.uint32), mo["fer"].view(np.uint32)), (what, key, "fer")
    assert np.array_equal(g["xcch"]["power"], m["xcch"]["power"]) and np.array_equal(g["xcch"]["ta"], m["xcch"]["ta"]), (what, "orders")
    for key in ("sch", "fcch"):
        for k in m[key]:
            assert np.array_equal(g[key][k], m[key][k]), (what, key, k, g[key][k][:12], m[key][k][:12])


def kind_of(name):
    """the TRXSIG_L1_* mapping kind a downlink mapping's name implies"""
    for prefix, kind in (("FACCH_TCHF", 0), ("SACCH_TF", 1), ("SDCCH_8", 2), ("SACCH_C8", 3), ("SDCCH_4", 4), ("SACCH_C4", 5),
                         ("CCCH", 7), ("BCCH", 8), ("SCH", 9), ("FCCH", 10)):
        if name.startswith(prefix):
            return kind
    raise ValueError(name)


def random_plan(rng, A):
    comb = rng.choice(np.array([0, 1, 1, 7], np.uint8), (A, 8))
    comb[0, 0] = 5
    return comb


def cell_soft(rng, tx, comb, bsic, band, fn, F, noise=0.3):
    """what a cell with this plan sends over [fn, fn + F) (tests/l1_mux_model.py, random payloads, SIs set) as soft values
    [8 F][A][148]; slots nobody writes are noise"""
    _, enc, _ = tm.encode_cell(rng, tx, fn, F, bsic=bsic, band=band, comb=comb)
    soft = fsm.soft_from_bits(rng, enc["bits"].transpose(1, 0, 2), noise)
    empty = enc["what"].T == 0
    soft[empty] = rng.random((int(empty.sum()), 148)).astype(np.float32)
    return soft


def run_and_compare(rx, model, feed, fn, wire, what):
    rx.decode(feed.res, fn % HYPER, wire=wire)
    g = as_model(rx.collect())
    m = model.decode(feed.col, fn % HYPER, wire=wire)
    assert_same(g, m, what)
    return g, m


# ---- 1 ----
@pytest.mark.parametrize("wire", [True, False])
def test_random_plans_and_streams(pkg, ctx, prims, tx, wire):
    rng = np.random.default_rng(1300 + wire)
    A, F = 3, 120
    comb = random_plan(rng, A)
    comb[1, 2], comb[2, 5] = 1, 7
    bsic, band = int(rng.integers(0, 64)), [900, 1800, 1900][1 + wire]
    model = lrm.Model(comb, bsic, band, prims=prims)
    rx = pkg.L1MsRx(ctx, comb, bsic, band)
    classes = (lrm.TCH, lrm.XCCH, lrm.CCCH, lrm.BCCH, lrm.SCH, lrm.FCCH)
    assert [rx.channels(c) for c in classes] == [len(model.ch[c]) for c in classes]
    for cls in classes:
        for i, ch in enumerate(model.ch[cls]):
            kind = rx.channel(cls, i)[2]
            assert rx.channel(cls, i)[:2] == (ch.a, ch.tn) and rx.channel(cls, i)[3] == ch.sub, (cls, i)
            assert kind == kind_of(ch.m.name), (cls, i, kind, ch.m.name)
    closed = [(lrm.TCH, 0), (lrm.XCCH, 1), (lrm.XCCH, 5), (lrm.CCCH, 2)]
    for cls, i in closed:
        rx.close(cls, i)
        model.ch[cls][i].active = False
    fn = int(rng.integers(0, HYPER - 2 * F))
    for call in range(2):
        soft = cell_soft(rng, tx, comb, bsic, band, fn, F)
        feed = Feed(pkg, rng, soft, rng.random((8 * F, A)) >= 0.15)
        g, m = run_and_compare(rx, model, feed, fn, wire, ("call", call))
        fn += F
        if call == 0:                                        # reopen: FER reset, SACCH orders back to 40 / 0
            for cls, i in closed[1:3]:
                rx.open(cls, i)
                model.ch[cls][i].open()
    assert (m["xcch"]["status"] & fsm.TCH_GOOD).any() and (m["tch"]["status"] & fsm.TCH_GOOD).any()
    assert (m["ccch"]["status"] & fsm.TCH_GOOD).any() and (m["bcch"]["status"] & fsm.TCH_GOOD).any()
    assert m["sch"]["sync"].any() and not m["sch"]["present"].all() and (m["fcch"]["ones"] == 0).any()
    assert (m["xcch"]["power"] > 0).any() and (m["xcch"]["power"] != 40).any()
    rx.destroy()


# ---- 2 ----
@pytest.mark.parametrize("fn0,F", [(5304 * 3 - 60, 120), (HYPER - 60, 150)])
def test_chaining_across_the_wraps(pkg, ctx, prims, tx, fn0, F):
    """One decode of F frames against the model, then the same input decoded in five pieces at random frame cuts by a second
    object: every block, the lists, the final state and the orders equal the whole call's."""
    rng = np.random.default_rng(fn0 % 1000)
    A = 2
    comb = random_plan(rng, A)
    comb[1, 3], comb[0, 2] = 1, 7
    model = lrm.Model(comb, 7, prims=prims)
    soft = cell_soft(rng, tx, comb, 7, 900, fn0, F)
    feed = Feed(pkg, rng, soft, rng.random((8 * F, A)) >= 0.15)
    whole = pkg.L1MsRx(ctx, comb, 7)
    gw, _ = run_and_compare(whole, model, feed, fn0, True, "whole")
    cuts = [0] + sorted(rng.choice(np.arange(1, F), 4, replace=False).tolist()) + [F]
    part = pkg.L1MsRx(ctx, comb, 7)
    blocks, lists = {}, []
    for lo, hi in zip(cuts, cuts[1:]):
        part.decode(feed.result(lo, hi), (fn0 + lo) % HYPER)
        g = as_model(part.collect())
        blocks.update(lrm.blocks_by_fn(g))
        lists.append(g)
    assert blocks == lrm.blocks_by_fn(gw) and len(blocks) > 50
    for key in BLOCK_KEYS:
        for k in ("state", "rssi", "timing"):
            assert np.array_equal(g[key][k], gw[key][k]), (key, k)
    assert np.array_equal(g["xcch"]["power"], gw["xcch"]["power"]) and np.array_equal(g["xcch"]["ta"], gw["xcch"]["ta"])
    for key in ("sch", "fcch"):
        for k in gw[key]:
            assert np.array_equal(np.concatenate([x[key][k] for x in lists]), gw[key][k]), (key, k)
    assert any(c % 4 for c in cuts) and (gw["sch"]["fn"] < 200).any() == (fn0 > HYPER // 2)
    whole.destroy(); part.destroy()


# ---- 3 ----
def test_lists_past_one_wave_and_one_finish_block(pkg, ctx, prims, tx):
    """One ARFCN with only the combination-V slot over 2,652 frames: 260 SCH and 260 FCCH entries (past a 64-lane chunk and a
    256-thread finish block), CCCH channels with 208 slots, 52 BCCH blocks."""
    rng = np.random.default_rng(1500)
    comb = np.zeros((1, 8), np.uint8); comb[0, 0] = 5
    fn, F = 51 * 7 + 3, 2652
    model = lrm.Model(comb, 33, prims=prims)
    soft = cell_soft(rng, tx, comb, 33, 900, fn, F)
    present = np.zeros((8 * F, 1), bool)
    present[0::8, 0] = rng.random(F) >= 0.15
    feed = Feed(pkg, rng, soft, present)
    rx = pkg.L1MsRx(ctx, comb, 33)
    g, m = run_and_compare(rx, model, feed, fn, True, "combination V alone")
    o = rx.out
    assert o.sch_cap == 260 and o.fcch_cap == 260 and o.nb_ctl >= 52 and (m["bcch"]["status"] & fsm.TCH_GOOD).sum() > 20
    assert m["sch"]["sync"].sum() > 150 and (m["sch"]["sync"][200:]).any() and set(np.unique(m["bcch"]["tc"])) == set(range(8))
    assert (m["fcch"]["ones"] == -1).sum() > 20 and (m["fcch"]["ones"][200:] == 0).any()
    rx.destroy()


def test_traffic_channels_past_one_wave(pkg, ctx, prims, tx):
    """2 ARFCNs of combination I over 104 frames: 96 slots per TCH channel"""
    rng = np.random.default_rng(1501)
    comb = np.ones((2, 8), np.uint8)
    fn, F = 26 * 1000 + 5, 104
    model = lrm.Model(comb, 3, prims=prims)
    soft = cell_soft(rng, tx, comb, 3, 900, fn, F)
    feed = Feed(pkg, rng, soft, rng.random((8 * F, 2)) >= 0.15)
    rx = pkg.L1MsRx(ctx, comb, 3)
    g, m = run_and_compare(rx, model, feed, fn, True, "combination I")
    assert 4 * rx.out.nb_tch >= 96 and (m["tch"]["status"] & fsm.TCH_GOOD).sum() > 50
    rx.destroy()


# ---- 4 ----
def test_sch_verdicts(pkg, ctx, prims):
    """Clean SCH bursts of trxsig_fec_sch_encode_batch at the slot's own FN: sync.  Another BSIC, or the burst of another SCH
    frame: ok, not sync.  20 flipped coded bits: not ok.  Noise rows and absent rows."""
    import torch
    rng = np.random.default_rng(1600)
    comb = np.zeros((1, 8), np.uint8); comb[0, 0] = 5
    bsic, fn, F = 37, HYPER - 130, 260
    model = lrm.Model(comb, bsic, prims=prims)
    frames = [k for k in range(F) if model.route(0, 0, (fn + k) % HYPER) is model.ch[lrm.SCH][0]]
    assert len(frames) >= 24
    kinds = np.arange(len(frames)) % 6                       # 0 clean, 1 other BSIC, 2 another frame's, 3 flipped, 4 noise, 5 absent
    enc_fn = np.array([(fn + frames[(j + 3) % len(frames)] if k == 2 else fn + f) % HYPER for j, (f, k) in enumerate(zip(frames, kinds))],
                      np.uint32)
    enc_bsic = np.where(kinds == 1, bsic ^ 0x21, bsic).astype(np.uint8)
    bits = torch.zeros(len(frames), 148, dtype=torch.uint8, device="cuda")
    ctx.fec_sch_encode(dev(enc_fn.astype(np.int32)), dev(enc_bsic), bits)
    bits = bits.cpu().numpy()
    flip = [3 + 2 * i for i in range(10)] + [106 + 3 * i for i in range(10)]
    soft = rng.random((8 * F, 1, 148)).astype(np.float32)
    present = np.zeros((8 * F, 1), bool)
    for j, (f, k) in enumerate(zip(frames, kinds)):
        b = bits[j].copy()
        if k == 3:
            b[flip] ^= 1
        if k != 4:
            soft[8 * f, 0] = b
        present[8 * f, 0] = k != 5
    feed = Feed(pkg, rng, soft, present, p_invalid=0.0)
    rx = pkg.L1MsRx(ctx, comb, bsic)
    g, m = run_and_compare(rx, model, feed, fn, True, "sch")
    s = g["sch"]
    assert np.array_equal(s["fn"], (fn + np.array(frames)) % HYPER)
    assert s["sync"][kinds == 0].all() and s["ok"][kinds == 0].all() and (s["rfn"][kinds == 0] == s["fn"][kinds == 0]).all()
    assert s["ok"][kinds == 1].all() and not s["sync"][kinds == 1].any() and (s["bsic"][kinds == 1] == bsic ^ 0x21).all()
    assert s["ok"][kinds == 2].all() and not s["sync"][kinds == 2].any() and (s["rfn"][kinds == 2] == enc_fn[kinds == 2]).all()
    assert not s["ok"][kinds == 3].any() and not s["sync"][kinds >= 3].any()
    assert s["present"][kinds != 5].all() and not s["present"][kinds == 5].any()
    for k in ("ok", "bsic", "rfn", "sync"):
        assert not s[k][kinds == 5].any()
    rx.destroy()


# ---- 5 ----
def test_bad_inputs(pkg, ctx):
    L = ctx.L
    ok = np.zeros((2, 8), np.uint8); ok[0, 0] = 5; ok[1, :] = 7; ok[0, 3] = 1
    pkg.L1MsRx(ctx, ok, 0).destroy()
    for bad in ([(1, 0, 5)], [(0, 1, 5)], [(0, 2, 4)], [(1, 3, 2)], [(0, 5, 9)]):
        comb = ok.copy()
        for a, tn, v in bad:
            comb[a, tn] = v
        h = C.c_void_p()
        assert L.trxsig_l1msrx_create(C.byref(h), ctx.h, 2, comb.ctypes.data, 0, 900) == EINVAL, bad
    h = C.c_void_p()
    assert L.trxsig_l1msrx_create(C.byref(h), ctx.h, 2, ok.ctypes.data, 64, 900) == EINVAL
    assert L.trxsig_l1msrx_create(C.byref(h), ctx.h, 2, ok.ctypes.data, 1, 1000) == EINVAL
    assert L.trxsig_l1msrx_create(C.byref(h), ctx.h, 2, None, 1, 900) == EINVAL
    assert L.trxsig_l1msrx_create(C.byref(h), ctx.h, 0, ok.ctypes.data, 1, 900) == EINVAL
    rx = pkg.L1MsRx(ctx, ok, 3)
    rng = np.random.default_rng(5)
    feed = Feed(pkg, rng, rng.random((16, 2, 148)).astype(np.float32), np.ones((16, 2), bool))
    out = pkg.L1MsRxOut()
    dec = lambda res, fn=0, o=out: L.trxsig_l1msrx_decode(rx.h, res, fn, 1, o)
    assert dec(C.byref(feed.res)) == 0
    for field, v in (("n_slots", 12), ("n_slots", 0), ("n_arfcn", 1), ("soft_stride", 100), ("d_row", None), ("n_rows", -1),
                     ("d_soft", None), ("d_valid", None), ("d_amp", None), ("d_toa", None)):
        r = pkg.TrxGroupResult(); C.pointer(r)[0] = feed.res
        setattr(r, field, v)
        assert dec(C.byref(r)) == EINVAL, field
    assert dec(C.byref(feed.res), fn=HYPER) == EINVAL and dec(C.byref(feed.res), fn=-1) == EINVAL
    assert dec(None) == EINVAL and dec(C.byref(feed.res), o=None) == EINVAL
    # classes: 2 is the uplink's RACH; SCH and FCCH have no active flag; channels out of range
    assert L.trxsig_l1msrx_channels(rx.h, 2) == EINVAL and L.trxsig_l1msrx_channels(rx.h, 7) == EINVAL
    assert [L.trxsig_l1msrx_channels(rx.h, c) for c in (0, 1, 3, 4, 5, 6)] == [1, 8 + 1 + 16 * 8, 3, 1, 1, 1]
    assert L.trxsig_l1msrx_open(rx.h, 2, 0) == EINVAL and L.trxsig_l1msrx_close(rx.h, 1, 10 ** 6) == EINVAL
    assert L.trxsig_l1msrx_open(rx.h, pkg.L1_SCH, 0) == EINVAL and L.trxsig_l1msrx_close(rx.h, pkg.L1_FCCH, 0) == EINVAL
    assert L.trxsig_l1msrx_close(rx.h, pkg.L1_BCCH, 0) == 0 and L.trxsig_l1msrx_open(rx.h, pkg.L1_BCCH, 0) == 0
    assert L.trxsig_l1msrx_channel(rx.h, 2, 0, None, None, None, None) == EINVAL
    assert L.trxsig_l1msrx_channel(rx.h, pkg.L1_CCCH, 3, None, None, None, None) == EINVAL
    p = C.c_void_p()
    assert L.trxsig_l1msrx_state(rx.h, pkg.L1_SCH, C.byref(p)) == EINVAL and L.trxsig_l1msrx_state(rx.h, 0, None) == EINVAL
    assert L.trxsig_l1msrx_state(rx.h, pkg.L1_BCCH, C.byref(p)) == 0 and p.value
    ctx.synchronize()
    rx.destroy()


# ---- 6, 7, 8: a live trxsig_l1tx ----
PLAN = np.array([[5, 1, 7, 0, 1, 0, 0, 0], [1, 7, 0, 0, 0, 1, 0, 0]], np.uint8)


class Cell:
    """A live downlink: L1Tx with SIs set and a sibling L1Rx whose SACCH state moves with a random uplink pull per call, so that
    the orders it sends move too."""

    def __init__(self, pkg, ctx, rng, prims, comb, bsic, band):
        import test_gpu_l1rx
        self.pkg, self.ctx, self.rng, self.comb, self.bsic, self.band = pkg, ctx, rng, comb, bsic, band
        self.tx = pkg.L1Tx(ctx, comb, bsic, band)
        self.ul = pkg.L1Rx(ctx, comb, bsic, band)
        self.ulm = ldm.Model(comb, bsic, band=band, prims=prims)
        self.Pull = test_gpu_l1rx.Pull
        self.walk = lmm.MuxModel(comb, bsic, band=band, oracle=object())   # the plan and the mappings' walk only
        self.si = rng.integers(0, 256, (4, 23)).astype(np.uint8)
        self.tx.set_si(self.si)
        self.walk.si = self.si

    def encode(self, fn, F):
        """one uplink pull into the sibling, then the downlink's frames [fn, fn + F) with random payloads"""
        p = self.Pull(self.pkg, self.rng, self.ulm, fn, F)
        self.ul.decode(p.res, fn)
        self.ctx.synchronize()
        self.grids = tm.random_grids(self.rng, self.walk, fn, F)
        t = {k: dev(v) for k, v in self.grids.items()}
        self.tx.encode(fn, F, sibling=self.ul, **t)
        r = self.tx.collect(state=False)
        r["_keep"] = (t, p)
        return r

    def destroy(self):
        self.tx.destroy(); self.ul.destroy()


def level_power(band, power):
    return lmm.POWER[band][lmm.encode_power(band, power)]


def decoded_orders(band, enc, sacch, n):
    """what the orders a trxsig_l1tx reports after a call decode to, per XCCH channel"""
    return [(level_power(band, int(enc["ms_power"][i])), int(np.float32(enc["ms_ta"][i] + np.float32(0.5)))) if i in sacch else (-1, -1)
            for i in range(n)]


def test_bit_level_closed_loop(pkg, ctx, prims):
    """L1Tx.encode (2 ARFCNs, 208 frames, SIs set, random payloads, two channels closed -- idle fill -- and one closed and
    reopened, a sibling L1Rx so that the orders move) -> d_bits as soft values -> L1MsRx.decode: every payload back, BCCH blocks
    carry the SI of their TC, every SCH entry syncs, every FCCH entry has no ones, idle-fill blocks are decoded and not good,
    and the SACCH orders are what the multiplexer's decode to."""
    rng = np.random.default_rng(1700)
    bsic, band, fn, F = 21, 900, 5304 * 5 - 100, 208
    cell = Cell(pkg, ctx, rng, prims, PLAN, bsic, band)
    closed = [(lmm.TCH, 1), (lmm.XCCH, 9)]
    for cls, i in closed:
        cell.tx.close(cls, i)
    cell.tx.close(lmm.CCCH, 1); cell.tx.open(lmm.CCCH, 1)
    enc = cell.encode(fn, F)
    assert (enc["what"] == pkg.L1TX_IDLE).sum() == 24 + 4
    model = lrm.Model(PLAN, bsic, band, prims=prims)
    feed = Feed(pkg, rng, fsm.soft_from_bits(rng, enc["bits"].transpose(1, 0, 2), 0.3), enc["what"].T != 0, p_invalid=0.0)
    rx = pkg.L1MsRx(ctx, PLAN, bsic, band)
    g, m = run_and_compare(rx, model, feed, fn, True, "bit level")
    n = tm.check_payloads(model, g, cell.walk, cell.grids, fn, F, cell.si, band, skip=closed)
    assert n["tch"] > 30 and n["xcch"] > 60 and n["ccch"] >= 9 and n["bcch"] >= 3, n
    assert g["sch"]["sync"].all() and len(g["sch"]["sync"]) >= 20 and (g["fcch"]["ones"] == 0).all() and len(g["fcch"]["ones"]) >= 20
    # idle fill: the blocks whose closing burst is a dummy burst
    idle = 0
    for cls, i in closed:
        key = "tch" if cls == lmm.TCH else "xcch"
        c = model.ch[lrm.TCH if cls == lmm.TCH else lrm.XCCH][i]
        for b, f in enumerate(g[key]["fn"][i]):
            k = (int(f) - fn) % HYPER
            st = int(g[key]["status"][i, b])
            if k < F and enc["what"][c.a, 8 * k + c.tn] == pkg.L1TX_IDLE:
                assert st & fsm.DECODED and not st & (fsm.TCH_GOOD | fsm.FACCH_OK), (key, i, b, st)
                idle += 1
            else:
                assert st == 0, (key, i, b, st)
    assert idle >= 4
    # orders: every SACCH block of this (first) call carries the call's orders
    sacch = [i for i, c in enumerate(model.ch[lrm.XCCH]) if c.sacch]
    want = decoded_orders(band, enc, sacch, len(model.ch[lrm.XCCH]))
    heard = [i for i in sacch if (g["xcch"]["status"][i] & fsm.TCH_GOOD).any()]
    assert len(heard) >= len(sacch) - 1
    for i in heard:
        assert (int(g["xcch"]["power"][i]), int(g["xcch"]["ta"][i])) == want[i], i
    assert len({want[i] for i in heard}) > 1 and any(want[i] != (level_power(band, 40), 0) for i in heard)
    rx.destroy(); cell.destroy()


def test_sample_level_closed_loop(pkg, prims):
    """The same encode at 104 frames -> trxsig_modulate_batch (guard 8 + (TN % 4 == 0)) -> a path gain, a delay of up to half a
    symbol and noise of sigma 0 or 0.02 per burst -> TrxGroup.pull with every used TN set to TSC on every frame -> L1MsRx.decode.
    Every BCCH / CCCH / XCCH / TCH burst is detected, the result equals the model fed with TrxGroup.collect(), every payload comes
    back.  SCH / FCCH / idle-fill slots: equality with the model only."""
    import torch
    from openbts_ttsou_amd import synth
    sps, bsic, band, fn, F = 4, 21, 900, 102 * 104 * 2, 104
    rng = np.random.default_rng(1800)
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    cell = Cell(pkg, ctx, rng, prims, PLAN, bsic, band)
    closed = [(lmm.XCCH, 9)]
    cell.tx.close(*closed[0])
    enc = cell.encode(fn, F)
    A, T = PLAN.shape[0], 8 * F
    sent = np.argwhere(enc["what"].T != 0)                    # (t, a) in time order
    bb = np.stack([enc["bits"][a, t] for t, a in sent])
    guard = np.array([8 + (t % 8 % 4 == 0) for t, _ in sent], np.int32)
    length = (sps * (148 + guard)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int32)
    mod = torch.zeros(int(length.sum()), 2, dtype=torch.float32, device="cuda")
    ctx.modulate(dev(bb), dev(guard), mod, dev(off))
    mod = mod.cpu().numpy().view(np.complex64).ravel()
    base = np.zeros((len(sent), 157 * sps), np.complex64)
    for i in range(len(sent)):
        base[i, :length[i]] = mod[off[i]:off[i] + length[i]]
    crng = np.random.default_rng(1801)
    xs, offs, lens, _, _ = synth._finish(crng, base, len(sent), sps, crng.uniform(-0.5, 0.5, len(sent)), (0.0, 0.02))
    cellw = 160 * sps
    x = np.zeros((T, A, cellw), np.complex64)
    for i, (t, a) in enumerate(sent):
        v = xs[offs[i]:offs[i] + lens[i]][:length[i]]
        x[t, a, :len(v)] = v
    grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn, 0))
    for a in range(A):
        for cmd in ["CMD RXTUNE 935000", "CMD TXTUNE 890000", "CMD SETTSC %d" % (bsic & 7)] + \
                   ["CMD SETSLOT %d %d" % (tn, 3 if PLAN[a, tn] else 0) for tn in range(8)] + ["CMD POWERON"]:
            grp.control(a, cmd)
    dx = torch.from_numpy(x.view(np.float32).reshape(-1)).to("cuda:0")
    res = grp.pull(dx.data_ptr(), A * cellw, cellw, fn, 0, T)
    grp.sync()
    rx = pkg.L1MsRx(ctx, PLAN, bsic, band)
    rx.decode(res, fn)
    g = as_model(rx.collect())
    col = grp.collect()
    normal = [pkg.L1TX_BCCH, pkg.L1TX_CCCH, pkg.L1TX_XCCH, pkg.L1TX_TCH]
    missed = [(t, a) for t, a in sent if enc["what"][a, t] in normal and not col["valid"][t, a]]
    assert not missed, ("a clean burst was not detected", missed[:5])
    model = lrm.Model(PLAN, bsic, band, prims=prims)
    assert_same(g, model.decode(col, fn), "sample level")
    n = tm.check_payloads(model, g, cell.walk, cell.grids, fn, F, cell.si, band, skip=closed)
    assert n["tch"] > 30 and n["xcch"] > 20 and n["ccch"] >= 3 and n["bcch"] >= 1, n
    rx.destroy(); cell.destroy(); grp.close(); ctx.close()


def test_follow(pkg, ctx, prims):
    """Two L1Ms over three rounds of 104 frames: one follows an L1MsRx fed from a live L1Tx, the other gets set_phy(c,
    ord_power[c], ord_ta[c]) for every open SACCH channel before each encode.  Bits, what, the handsets and the records are
    equal byte for byte; then the TRXSIG_EINVAL cases of trxsig_l1ms_follow."""
    import l1_ms_model as lms
    rng = np.random.default_rng(1900)
    bsic, band, F = 13, 900, 104
    fn = 102 * 104 * 3
    cell = Cell(pkg, ctx, rng, prims, PLAN, bsic, band)
    rx = pkg.L1MsRx(ctx, PLAN, bsic, band)
    a, b = pkg.L1Ms(ctx, PLAN, bsic, band), pkg.L1Ms(ctx, PLAN, bsic, band)
    a.follow(rx)
    walk = lms.MsModel(PLAN, bsic, band, oracle=object())    # plan and walk only
    sacch = [i for i, c in enumerate(walk.ch[lms.XCCH]) if c.sacch]
    shut = sacch[2]
    a.close(lms.XCCH, shut); b.close(lms.XCCH, shut)
    content = lms.Content(rng, p_none=0.1, speech=True)
    seen = set()
    for rnd in range(3):
        enc = cell.encode(fn, F)
        feed = Feed(pkg, rng, fsm.soft_from_bits(rng, enc["bits"].transpose(1, 0, 2), 0.25), enc["what"].T != 0, p_invalid=0.0)
        rx.decode(feed.res, fn)
        o = rx.collect(state=False)
        for i in sacch:
            if i != shut:
                b.set_phy(i, int(o["ord_power"][i]), int(o["ord_ta"][i]))
        g = {k: dev(v) for k, v in lms.grids(walk, content, fn, F).items()}
        a.encode(fn, F, **g)
        b.encode(fn, F, **g)
        ra, rb = a.collect(), b.collect()
        for k in ("bits", "what", "ms_power", "ms_ta", "tch_state", "xcch_state"):
            assert np.array_equal(ra[k], rb[k]), (rnd, k)
        assert (int(ra["ms_power"][shut]), int(ra["ms_ta"][shut])) == (level_power(band, 40), 0)
        seen |= {(int(p), int(t)) for p, t in zip(ra["ms_power"][sacch], ra["ms_ta"][sacch])}
        fn += F
    assert len(seen) > 1 and (ra["what"] != 0).sum() > 500
    # the bad-input rules
    L = ctx.L
    ins, out = pkg.L1MsIn(), pkg.L1MsOut()
    for name, t in zip(("d_tch_kind", "d_tch_payload", "d_xcch_kind", "d_xcch_payload", "d_rach_kind", "d_rach_ra"),
                       (g["tch_kind"], g["tch_payload"], g["xcch_kind"], g["xcch_payload"], g["rach_kind"], g["rach_ra"])):
        setattr(ins, name, t.data_ptr())
    assert L.trxsig_l1ms_encode(a.h, fn, F, C.byref(ins), cell.tx.h, C.byref(out)) == EINVAL     # a sibling while following
    assert L.trxsig_l1ms_encode(b.h, fn, F, C.byref(ins), cell.tx.h, C.byref(out)) == 0
    assert L.trxsig_l1ms_follow(None, rx.h) == EINVAL
    other = PLAN.copy(); other[1, 6] = 1
    rx2 = pkg.L1MsRx(ctx, other, bsic, band)
    rx3 = pkg.L1MsRx(ctx, PLAN, bsic ^ 1, band)
    rx4 = pkg.L1MsRx(ctx, PLAN, bsic, 1800)
    ctx2 = pkg.TrxSig(4, 0)
    rx5 = pkg.L1MsRx(ctx2, PLAN, bsic, band)
    for r in (rx2, rx3, rx4, rx5):
        assert L.trxsig_l1ms_follow(b.h, r.h) == EINVAL
    assert L.trxsig_l1ms_follow(b.h, rx.h) == 0 and L.trxsig_l1ms_follow(b.h, None) == 0 and L.trxsig_l1ms_follow(a.h, None) == 0
    assert L.trxsig_l1ms_encode(a.h, fn, F, C.byref(ins), cell.tx.h, C.byref(out)) == 0          # no longer following
    ctx.synchronize()
    for r in (rx, rx2, rx3, rx4, rx5):
        r.destroy()
    a.destroy(); b.destroy(); cell.destroy(); ctx2.close()
