"""GPU parity of the hopping stage (trxsig_l1hop.h) against its model (tests/l1_hop_model.py): the primitive on the known answers
and on random entries; map() across the T1R wrap and the hyperframe wrap; bits() in both directions byte for byte, without the
map, split at a frame boundary, there and back, with sentinels after the grid; cells() word for word on both access widths and
both nestings with guard words; result(); the closed loop at L1 on the downlink and through samples on the uplink, with one
frequency silenced; the bad-input rules.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _pkg
import fec_stream_model as fsm
import l1_ciph_model as lcm
import l1_hop_model as lhm
import l1_ms_model as lms
import test_gpu_l1ciph as tci

pytestmark = pytest.mark.gpu
HYPER = lhm.HYPERFRAME
EINVAL = -1
GOOD = fsm.DECODED | fsm.TCH_GOOD
FN_T1R = 1326 * 64 - 3                                       # T1R goes 63 -> 0 three frames in
dev = tci.dev


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.TrxSig(4, 0)
    c.use_torch_stream()
    yield c


@pytest.fixture(scope="module")
def ctx1(pkg):
    c = pkg.TrxSig(1, 0)
    c.use_torch_stream()
    yield c


PLANS = {"small": lhm.small_plan, "big": lhm.big_plan}


@pytest.fixture(scope="module", params=["small", "big"])
def hop(request, pkg, ctx):
    comb, group, hsn = PLANS[request.param]()
    h, m = pkg.L1Hop(ctx, comb, group, hsn, max_frames=16), lhm.HopModel(comb, group, hsn)
    yield h, m
    h.destroy()


# ---- 1: the primitive ----
def test_primitive(pkg, ctx):
    import torch
    i32 = lambda v: dev(np.asarray(v, np.int32))
    for (hsn, maio, n), fns, want in (((1, 0, 4), range(0, 20), [2, 0, 3, 2, 3, 3, 2, 0, 1, 1, 2, 3, 1, 1, 1, 3, 3, 1, 0, 0]),
                                      ((63, 2, 64), range(83578, 83590), [47, 41, 7, 57, 45, 9, 6, 52, 35, 34, 35, 11])):
        k = len(want)
        out = torch.full((k,), -7, dtype=torch.int32, device="cuda")
        pkg.hop_mai(ctx, i32(list(fns)), i32([hsn] * k), i32([maio] * k), i32([n] * k), out)
        ctx.synchronize()
        assert out.cpu().tolist() == want
    rng = np.random.default_rng(11)
    cnt = 4099                                               # 64 waves and three lanes: a workgroup boundary, a wave boundary, a lane
    n = rng.integers(1, 65, cnt)
    n[:8] = [1, 2, 63, 64, 64, 33, 32, 1]
    maio = (rng.integers(0, 64, cnt) % n)
    hsn = rng.integers(0, 64, cnt)
    hsn[8:40] = 0
    fn = rng.integers(0, HYPER, cnt)
    fn[:6] = [0, HYPER - 1, 84863, 84864, 83577, 1325]
    want = lhm.mai_batch(fn, hsn, maio, n)
    SENT = -12345
    out = torch.full((cnt + 64,), SENT, dtype=torch.int32, device="cuda")
    pkg.hop_mai(ctx, i32(fn), i32(hsn), i32(maio), i32(n), out)
    ctx.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:cnt], want) and (got[cnt:] == SENT).all() and len(set(want.tolist())) > 40
    L = ctx.L
    assert L.trxsig_hop_mai_batch(ctx.h, 0, None, None, None, None, None) == 0
    d = [i32(fn).data_ptr()] * 4 + [out.data_ptr()]
    for bad in ([-1] + d, [1 << 25] + d, [cnt, None] + d[1:], [cnt] + d[:3] + [None, d[4]], [cnt] + d[:4] + [None]):
        assert L.trxsig_hop_mai_batch(ctx.h, *bad) == EINVAL
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), got)


# ---- 2: the plan and the map ----
def test_plan_queries_and_map(pkg, ctx, hop):
    h, m = hop
    assert h.groups() == m.groups()
    for g in range(m.groups()):
        for tn in range(8):
            assert h.members(g, tn) == m.members(g, tn), (g, tn)
    for fn in (FN_T1R, HYPER - 2):
        got = h.map(fn, 6)
        ctx.synchronize()
        want = m.map(fn, 6)
        assert np.array_equal(got.cpu().numpy(), want), fn
        assert (want != np.arange(m.A)).sum() > 20


# ---- 3: bits ----
def test_bits_against_the_model(pkg, ctx, hop):
    import torch
    h, m = hop
    A, F, fn = m.A, 6, FN_T1R
    T = 8 * F
    rng = np.random.default_rng(21 + A)
    bits = rng.integers(0, 2, (A, T, 148)).astype(np.uint8)
    what = rng.integers(0, 8, (A, T)).astype(np.uint8)
    SENT, PAD = 0xA5, 512
    nb, nw = bits.size, what.size

    def padded(x):
        buf = torch.full((x.size + PAD,), SENT, dtype=torch.uint8, device="cuda")
        buf[:x.size] = dev(x).reshape(-1)
        return buf

    for to_radio in (1, 0):
        wb, ww = m.bits(to_radio, fn, F, bits, what)
        assert (wb != bits).any(-1).sum() > 30 and (ww != what).sum() > 20
        db, dw = padded(bits), padded(what)
        h.bits(to_radio, fn, F, db, dw)
        ctx.synchronize()
        gb, gw = db.cpu().numpy(), dw.cpu().numpy()
        assert np.array_equal(gb[:nb].reshape(bits.shape), wb), to_radio
        assert np.array_equal(gw[:nw].reshape(what.shape), ww), to_radio
        assert (gb[nb:] == SENT).all() and (gw[nw:] == SENT).all()
        # there and back is the identity
        h.bits(1 - to_radio, fn, F, db, dw)
        ctx.synchronize()
        assert np.array_equal(db.cpu().numpy()[:nb].reshape(bits.shape), bits) and np.array_equal(dw.cpu().numpy()[:nw].reshape(what.shape), what)
        # d_what NULL: the grid alone
        db = padded(bits)
        h.bits(to_radio, fn, F, db, None)
        # 2 + 4 frames equal one call
        parts = [(padded(bits[:, 8 * lo:8 * hi]), padded(what[:, 8 * lo:8 * hi]), lo, hi) for lo, hi in ((0, 2), (2, 6))]
        for pb, pw, lo, hi in parts:
            h.bits(to_radio, (fn + lo) % HYPER, hi - lo, pb, pw)
        ctx.synchronize()
        assert np.array_equal(db.cpu().numpy()[:nb].reshape(bits.shape), wb)
        cat = lambda i, shape: np.concatenate([p[i].cpu().numpy()[:-PAD].reshape((A, 8 * (p[3] - p[2])) + shape) for p in parts], axis=1)
        assert np.array_equal(cat(0, (148,)), wb) and np.array_equal(cat(1, ()), ww)
        assert all((p[i].cpu().numpy()[-PAD:] == SENT).all() for p in parts for i in (0, 1))
    # across the hyperframe wrap
    wb, ww = m.bits(1, HYPER - 2, F, bits, what)
    db, dw = padded(bits), padded(what)
    h.bits(1, HYPER - 2, F, db, dw)
    ctx.synchronize()
    assert np.array_equal(db.cpu().numpy()[:nb].reshape(bits.shape), wb) and np.array_equal(dw.cpu().numpy()[:nw].reshape(what.shape), ww)


# ---- 4: cells ----
@pytest.mark.parametrize("sps,even", [(1, False), (1, True), (4, True), (4, False)])
@pytest.mark.parametrize("to_radio", [1, 0])
def test_cells_against_the_model(pkg, ctx, ctx1, sps, even, to_radio):
    """Random 32-bit words (NaN payloads among them) in the cells and in the guards; the whole destination, guards and the words
    after the grid included, against the model as 64-bit words.  sps 1 with odd strides takes the 8-byte path, even strides the
    16-byte path (sps 1: with the odd cells' last sample on its own); slot-major into ARFCN-major and back."""
    import torch
    c = ctx1 if sps == 1 else ctx
    comb, group, hsn = lhm.small_plan()
    h, m = pkg.L1Hop(c, comb, group, hsn), lhm.HopModel(comb, group, hsn)
    A, F, fn = m.A, 6, FN_T1R
    T = 8 * F
    rng = np.random.default_rng(31 + sps + 2 * even + 4 * to_radio)
    cell = 157 * sps + (3 if even else 4)
    cell += (cell & 1) != (0 if even else 1)                 # even / odd as asked
    lay_a = (A * cell + (2 if even else 4), cell)            # slot-major: (slot stride, row stride)
    lay_b = (cell, T * cell + (6 if even else 1))            # row-major
    assert all((x & 1) == (0 if even else 1) for x in lay_a + lay_b)
    (isl, iar), (osl, oar) = (lay_a, lay_b) if to_radio else (lay_b, lay_a)
    n_in = (T - 1) * isl + (A - 1) * iar + 157 * sps
    n_out = (T - 1) * osl + (A - 1) * oar + 157 * sps + 64    # and 64 samples after the grid
    src = rng.integers(0, 1 << 32, 2 * n_in, dtype=np.uint64).astype(np.uint32)
    dst0 = rng.integers(0, 1 << 32, 2 * n_out, dtype=np.uint64).astype(np.uint32)
    assert np.isnan(src.view(np.float32)).sum() > 10
    want = m.cells(to_radio, fn, F, src.view(np.uint64), isl, iar, dst0.view(np.uint64).copy(), osl, oar, sps)
    dsrc, ddst = dev(src.view(np.int32)), dev(dst0.view(np.int32))
    assert dsrc.data_ptr() % 16 == 0 and ddst.data_ptr() % 16 == 0
    h.cells(to_radio, fn, F, dsrc, isl, iar, ddst, osl, oar)
    c.synchronize()
    got = ddst.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert (want != dst0.view(np.uint64)).sum() > T * A * 150 * sps and np.array_equal(got[-64:], dst0.view(np.uint64)[-64:])
    assert np.array_equal(dsrc.cpu().numpy().view(np.uint32), src)
    if even and sps == 1:                                     # a base that is 8 but not 16 bytes aligned: the 8-byte path again
        ddst2 = dev(np.concatenate([np.zeros(2, np.uint32), dst0]).view(np.int32))
        h.cells(to_radio, fn, F, dsrc, isl, iar, ddst2.data_ptr() + 8, osl, oar)
        c.synchronize()
        assert np.array_equal(ddst2.cpu().numpy().view(np.uint32)[2:].view(np.uint64), want)
    # overlap, and strides under which cells overlap: TRXSIG_EINVAL, nothing written
    L = c.L
    p, q = dsrc.data_ptr(), ddst.data_ptr()
    for args in ((p, isl, iar, p, isl, iar), (p, isl, iar, p + 8 * (n_in - 1), osl, oar), (p, isl, iar, q, 157 * sps - 1, oar),
                 (p, 10, 10, q, osl, oar), (None, isl, iar, q, osl, oar), (p, isl, iar, None, osl, oar)):
        assert L.trxsig_l1hop_cells(h.h, to_radio, fn, F, *args) == EINVAL, args
    c.synchronize()
    assert np.array_equal(ddst.cpu().numpy().view(np.uint64), want) and np.array_equal(dsrc.cpu().numpy().view(np.uint32), src)
    h.destroy()


# ---- 5: result ----
def test_result_against_the_model(pkg, ctx, hop):
    h, m = hop
    A, F, fn = m.A, 6, HYPER - 2
    T = 8 * F
    rng = np.random.default_rng(41 + A)
    row = rng.permutation(T * A).astype(np.int32).reshape(T, A)
    row[rng.random((T, A)) < 0.2] = -1
    res, keep = tci.make_result(pkg, row, np.full(T * A, 2, np.uint8), np.zeros((T * A, 148), np.float32))
    out = h.result(res, fn)
    ctx.synchronize()
    got = h.row.cpu().numpy()                                # the object's array, as a tensor
    want = m.result(fn, row)
    assert np.array_equal(got, want) and (want != row).sum() > 20
    assert np.array_equal(keep["row"].cpu().numpy(), row)      # res's own array is only read
    assert out.d_row != res.d_row
    for f, _ in pkg.TrxGroupResult._fields_:
        if f != "d_row":
            assert getattr(out, f) == getattr(res, f), f


# ---- 6: the closed loop at L1, downlink ----
def downlink_leg(pkg, ctx, comb, group, hsn, fn, F, grids, keys, hop_tx=True, dehop=True):
    """l1tx_encode -> l1ciph_bits -> [l1hop_bits] -> soft rows and a result -> [l1hop_result] -> l1ciph_soft -> l1msrx_decode"""
    bsic = 21
    enc, dec, ci = pkg.L1Tx(ctx, comb, bsic), pkg.L1MsRx(ctx, comb, bsic), pkg.L1Ciph(ctx, comb)
    hp = pkg.L1Hop(ctx, comb, group, hsn, max_frames=F)
    for (cls, i), kc in keys.items():
        ci.set(cls, i, pkg.A5_1, kc)
    out = enc.encode(fn, F, **{k: dev(v) for k, v in grids.items()})
    ci.bits(0, fn, F, out.d_bits, out.d_what, 1 << pkg.L1TX_XCCH | 1 << pkg.L1TX_TCH)
    if hop_tx:
        hp.bits(1, fn, F, out.d_bits, out.d_what)            # the encoder's own grid and map, in place
    r = enc.collect(state=False)
    res, keep = tci.soft_result(pkg, r["bits"], r["what"])
    use = hp.result(res, fn) if (hop_tx and dehop) else res
    ci.soft(0, use, fn)
    dec.decode(use, fn)
    got = dec.collect(state=False)
    got["_what"], got["_bits"] = r["what"], r["bits"]
    info = {cls: [enc.channel(cls, i) for i in range(enc.channels(cls))] for cls in (pkg.L1_TCH, pkg.L1_XCCH)}
    for o in (enc, dec, ci, hp):
        o.destroy()
    return got, info


def test_closed_loop_downlink_at_l1(pkg, ctx):
    rng = np.random.default_rng(61)
    comb, group, hsn = lhm.small_plan()
    F, fn = 104, 1326 * 5 + 26
    tx = pkg.L1Tx(ctx, comb, 21)
    nbt, nbx, nbc = tx.grid(fn, F)
    nt, nx, nc = tx.channels(pkg.L1_TCH), tx.channels(pkg.L1_XCCH), tx.channels(pkg.L1_CCCH)
    tx.destroy()
    pay = rng.integers(0, 256, (nt, nbt, 33)).astype(np.uint8)
    pay[..., 32] &= 0xF0
    grids = dict(tch_kind=rng.choice(np.array([1, 1, 2], np.uint8), (nt, nbt)), tch_payload=pay,
                 xcch_kind=np.ones((nx, nbx), np.uint8), xcch_payload=rng.integers(0, 256, (nx, nbx, 23)).astype(np.uint8),
                 ccch_kind=np.ones((nc, nbc), np.uint8), ccch_payload=rng.integers(0, 256, (nc, nbc, 23)).astype(np.uint8))
    keys = {(lcm.TCH, i): rng.integers(1, 256, 8).astype(np.uint8) for i in range(nt)}
    keys.update({(lcm.XCCH, i): rng.integers(1, 256, 8).astype(np.uint8) for i in range(nx)})
    plain, info = downlink_leg(pkg, ctx, comb, group, hsn, fn, F, grids, keys, hop_tx=False)
    both, _ = downlink_leg(pkg, ctx, comb, group, hsn, fn, F, grids, keys)
    raw, _ = downlink_leg(pkg, ctx, comb, group, hsn, fn, F, grids, keys, dehop=False)
    xg = plain["xcch_status"] == GOOD
    tg = (plain["tch_status"] == GOOD) | ((plain["tch_status"] & fsm.FACCH_OK) != 0)
    assert xg.sum() > 60 and tg.sum() > 100 and tg.any(axis=1).all()
    assert (both["_bits"] != plain["_bits"]).any(-1).sum() > 500      # the bursts did move ...
    for k in tci.OUT_KEYS:                                     # ... and every payload comes back
        assert np.array_equal(both[k], plain[k]), k
    # the dehop left out: parity fails on the hopping channels with N > 1 and on no other.  A decoder then gets, in every slot
    # that moved, another channel's burst under another key: garbage on that burst's 114 positions.  One such burst in four
    # is sometimes corrected (the stream model: 7 of 2,400), two or more never are; a block none of whose bursts moved is the
    # plain run's.  So: every speech / FACCH channel (24 blocks of 8 bursts) loses blocks; of the combination-VII slots' blocks,
    # whose four bursts are the closing frame and the three before it, those with two or more moved bursts fail and those with
    # none are the plain run's.
    m = lhm.HopModel(comb, group, hsn)
    radio = m.map(fn, F)
    hops = lambda a, tn: group[a, tn] >= 0 and len(m.members(group[a, tn], tn)) > 1
    n_hop = 0
    for i, (a, tn, _, _) in enumerate(info[pkg.L1_TCH]):
        if hops(a, tn):
            bad = (raw["tch_status"][i] & (fsm.TCH_GOOD | fsm.FACCH_OK)) == 0
            assert (radio[tn::8, a] != a).sum() > F // 4 and (tg[i] & bad).sum() >= 4, i
            n_hop += 1
        else:
            for k in ("tch_status", "tch", "facch", "tch_fn"):
                assert np.array_equal(raw[k][i], plain[k][i]), (k, i)
    assert n_hop == 7
    n_hop = n_fail = n_same = 0
    for i, (a, tn, _, _) in enumerate(info[pkg.L1_XCCH]):
        if not hops(a, tn):
            for k in ("xcch_status", "xcch", "xcch_fn"):
                assert np.array_equal(raw[k][i], plain[k][i]), (k, i)
            continue
        n_hop += 1
        if comb[a, tn] != 7:
            continue
        for b in np.flatnonzero(xg[i]):
            k = (int(plain["xcch_fn"][i, b]) - fn) % HYPER
            moved = sum(int(radio[8 * (k - j) + tn, a] != a) for j in range(4))
            if moved >= 2:
                assert not raw["xcch_status"][i, b] & fsm.TCH_GOOD, (i, b)
                n_fail += 1
            elif moved == 0:
                assert raw["xcch_status"][i, b] == GOOD and np.array_equal(raw["xcch"][i, b], plain["xcch"][i, b]), (i, b)
                n_same += 1
    assert n_hop == 3 * 16 + 7 and n_fail > 30 and n_same >= 1


# ---- 7: the closed loop through samples, uplink, sps 1 ----
def dehop_collect(m, fn, col):
    """a TrxGroup.collect() in the channel domain, by the model"""
    T = col["valid"].shape[0]
    radio = m.map(fn, T // 8).astype(np.int64)
    return {k: (None if v is None else np.take_along_axis(v, radio.reshape(radio.shape + (1,) * (v.ndim - 2)), axis=1))
            for k, v in col.items()}


def test_closed_loop_uplink_through_samples(pkg, ctx1):
    """l1ms_encode -> radiate -> l1hop_cells -> trxsig_air_cells (one tap, no noise) -> pull -> l1hop_result -> l1rx_decode at sps 1:
    what is decoded equals the run without hopping.  Then radio row 2 -- a frequency of the N = 3 group of SDCCH/8 slots -- is
    silenced by zero taps: everything decoded equals the demultiplexer's model (the stream decoders' model inside it) on the
    pull's own bursts with those slots missing, the channels of the group lose blocks and keep others."""
    import torch
    import l1_demux_model as ldm
    import test_gpu_l1ms as tms
    import test_gpu_l1rx
    ctx = ctx1
    sps, F, fn0, bsic, band = 1, 104, 26 * 40, 21, 1800
    comb, group, hsn = lhm.small_plan()
    A, T = comb.shape[0], 8 * F
    m = lhm.HopModel(comb, group, hsn)
    model = lms.MsModel(comb, bsic, band, oracle=object())
    rng = np.random.default_rng(71)
    g = lms.grids(model, lms.Content(rng, p_none=0.0, speech=True), fn0, F)
    half = lambda n: rng.uniform(-0.5, 0.5, n) / sps
    chan = tms.Air(rng, model, len(g["rach_kind"]), half, half)
    prims = fsm.Prims()
    cell = 160 * sps
    silent = 2
    runs = {}
    for name in ("plain", "hop", "lost"):
        ms, rx = pkg.L1Ms(ctx, comb, bsic, band), pkg.L1Rx(ctx, comb, bsic, band)
        hp, air = pkg.L1Hop(ctx, comb, group, hsn, max_frames=F), pkg.Air(ctx, 1)
        ms.encode(fn0, F, **{k: tms.dev(v) for k, v in g.items()})
        r = ms.collect(state=False)
        buf = torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda")
        ms.radiate(buf, A * cell, cell, **chan.kwargs())
        if name == "plain":
            rad = buf
        else:
            rad = torch.zeros_like(buf)
            hp.cells(1, fn0, F, buf, A * cell, cell, rad, A * cell, cell)
        taps = np.ones((A, T, 1), np.complex64)
        if name == "lost":
            taps[silent] = 0
        air.cells(fn0, A, F, 0, rad, A * cell, cell, taps=dev(taps.view(np.float32).reshape(A, T, 1, 2)))
        grp = tms.setup_group(pkg, ctx, comb, bsic & 7, fn0)
        res = grp.pull(rad.data_ptr(), A * cell, cell, fn0, 0, T)
        grp.sync()
        use = res if name == "plain" else hp.result(res, fn0)
        rx.decode(use, fn0)
        got = rx.collect()
        col = grp.collect()
        sent = r["what"].T != 0                                # [T][A], the channel domain
        radio = m.map(fn0, F) if name != "plain" else np.tile(np.arange(A), (T, 1))
        on_air = np.zeros((T, A), bool)
        on_air[np.arange(T)[:, None].repeat(A, 1)[sent], radio[sent]] = True
        if name == "lost":
            assert on_air[:, silent].sum() > 100 and not col["valid"][:, silent].any()
            on_air[:, silent] = False
        assert col["valid"][on_air].all(), "a clean burst was not detected"
        if name != "plain":
            rxm = ldm.Model(comb, bsic, band=band, prims=prims)
            test_gpu_l1rx.assert_same(got, rxm.decode(dehop_collect(m, fn0, col), fn0), name)
        runs[name] = got
        for o in (ms, rx, hp, air):
            o.destroy()
        grp.close()
    plain, hopd, lost = runs["plain"], runs["hop"], runs["lost"]
    xg = plain["xcch_status"] == GOOD
    tg = (plain["tch_status"] == GOOD) | ((plain["tch_status"] & fsm.FACCH_OK) != 0)
    assert xg.sum() > 100 and tg.sum() > 100
    for k in ("tch_status", "tch_fn", "xcch_status", "xcch_fn", "xcch"):
        assert np.array_equal(plain[k], hopd[k]), k
    assert np.array_equal(plain["tch"][tg], hopd["tch"][tg]) and np.array_equal(plain["facch"][tg], hopd["facch"][tg])
    assert np.array_equal(plain["rach"]["ra"], hopd["rach"]["ra"]) and len(plain["rach"]["ra"]) > 10
    # the silenced frequency: the SDCCH channels of all three rows of the group lose some blocks and keep some; what is kept is
    # the plain run's; the channels that never use radio row 2 are the plain run's throughout
    lg = lost["xcch_status"] == GOOD
    assert not (lg & ~xg).any() and np.array_equal(lost["xcch"][lg], plain["xcch"][lg])
    touches = lambda c: (c.tn == 1 and c.a in (0, 2, 5)) or (c.tn == 4 and c.a in (2, 5))      # the groups radio row 2 is in
    sd = np.array([c.tn == 1 and c.a in (0, 2, 5) and not c.sacch for c in model.ch[lms.XCCH]])
    assert sd.sum() == 24 and 0 < lg[sd].sum() < xg[sd].sum() and lg[sd].any(axis=1).sum() >= 12
    for i, c in enumerate(model.ch[lms.XCCH]):
        if not touches(c):
            assert np.array_equal(lg[i], xg[i]), i
    on2 = np.array([c.a == silent or (c.tn == 4 and c.a == 5) for c in model.ch[lms.TCH]])      # rows whose slots visit radio row 2
    ltg = (lost["tch_status"] == GOOD) | ((lost["tch_status"] & fsm.FACCH_OK) != 0)
    assert np.array_equal(ltg[~on2], tg[~on2]) and (ltg[on2].sum(axis=1) < tg[on2].sum(axis=1)).all()


# ---- 8: the bad-input rules ----
def test_bad_inputs(pkg, ctx):
    """Each returns TRXSIG_EINVAL with nothing launched."""
    import torch
    L = ctx.L
    comb, group, hsn = lhm.small_plan()

    def create(c, g, hs, n_groups=None, max_frames=8, A=None):
        c, g, hs = np.ascontiguousarray(c, np.uint8), np.ascontiguousarray(g, np.int8), np.ascontiguousarray(hs, np.uint8)
        h = C.c_void_p()
        rc = L.trxsig_l1hop_create(C.byref(h), ctx.h, c.shape[0] if A is None else A, c.ctypes.data, g.ctypes.data,
                                   len(hs) if n_groups is None else n_groups, hs.ctypes.data if len(hs) else None, max_frames)
        if rc == 0:
            L.trxsig_l1hop_destroy(h)
        else:
            assert not h.value
        return rc

    assert create(comb, group, hsn) == 0
    g = group.copy(); g[0, 0] = 0; assert create(comb, g, hsn) == EINVAL                 # the beacon slot
    g = group.copy(); g[6, 1] = 0; assert create(comb, g, hsn) == EINVAL                 # an OFF slot
    c = comb.copy(); c[2, 1] = 1; assert create(c, group, hsn) == EINVAL                 # members of one allocation differ
    g = group.copy(); g[1, 3] = 4; assert create(comb, g, hsn) == EINVAL                 # group id out of range
    g = group.copy(); g[1, 3] = -2; assert create(comb, g, hsn) == EINVAL
    assert create(comb, group, [5, 0, 64, 17]) == EINVAL                                 # HSN
    assert create(comb, group, hsn, n_groups=3) == EINVAL and create(comb, group, hsn, n_groups=129) == EINVAL
    c = comb.copy(); c[1, 7] = 4; assert create(c, group, hsn) == EINVAL                 # a combination the plan does not know
    c65, g65 = np.ones((65, 8), np.uint8), np.full((65, 8), -1, np.int8)
    g65[:, 6] = 0
    assert create(c65, g65, [1]) == EINVAL                                               # N = 65
    g65[64, 6] = -1
    assert create(c65, g65, [1]) == 0
    assert create(comb, group, hsn, max_frames=0) == EINVAL and create(comb, group, hsn, max_frames=1 << 28) == EINVAL
    assert create(comb, group, hsn, A=0) == EINVAL
    assert create(comb, np.full_like(group, -1), [], n_groups=0) == 0                    # nothing hops: a legal plan
    h = C.c_void_p()
    assert L.trxsig_l1hop_create(C.byref(h), ctx.h, 7, None, group.ctypes.data, 4, hsn.ctypes.data, 8) == EINVAL
    assert L.trxsig_l1hop_create(C.byref(h), ctx.h, 7, comb.ctypes.data, None, 4, hsn.ctypes.data, 8) == EINVAL
    assert L.trxsig_l1hop_create(C.byref(h), ctx.h, 7, comb.ctypes.data, group.ctypes.data, 4, None, 8) == EINVAL and not h.value

    hp = pkg.L1Hop(ctx, comb, group, hsn, max_frames=2)
    assert L.trxsig_l1hop_members(hp.h, 4, 0, None) == EINVAL and L.trxsig_l1hop_members(hp.h, 0, 8, None) == EINVAL
    assert L.trxsig_l1hop_members(hp.h, -1, 0, None) == EINVAL and L.trxsig_l1hop_members(hp.h, 0, 1, None) == 3
    p = C.c_void_p()
    for fn, F, out in ((-1, 2, C.byref(p)), (HYPER, 2, C.byref(p)), (0, 0, C.byref(p)), (0, 3, C.byref(p)), (0, 2, None)):
        assert L.trxsig_l1hop_map(hp.h, fn, F, out) == EINVAL, (fn, F)
    src = np.arange(7 * 16 * 148, dtype=np.int64).astype(np.uint8).reshape(7, 16, 148)
    d = dev(src)
    a = d.data_ptr()
    for fn, F, ptr in ((-1, 2, a), (HYPER, 2, a), (0, 0, a), (0, -3, a), (0, 1 << 27, a), (0, 2, None), (0, 2, a + 2)):
        assert L.trxsig_l1hop_bits(hp.h, 1, fn, F, ptr, None) == EINVAL, (fn, F)
    x = torch.zeros(16 * 7 * 640, 2, dtype=torch.float32, device="cuda")
    y = torch.ones_like(x)
    for fn, F in ((-1, 2), (HYPER, 2), (0, 0), (0, 1 << 27)):
        assert L.trxsig_l1hop_cells(hp.h, 1, fn, F, x.data_ptr(), 7 * 640, 640, y.data_ptr(), 7 * 640, 640) == EINVAL, (fn, F)
    row = np.arange(112, dtype=np.int32).reshape(16, 7)
    res, t = tci.make_result(pkg, row, np.full(112, 2, np.uint8), np.ones((112, 148), np.float32))
    out = pkg.TrxGroupResult()
    for field, v in (("n_slots", 12), ("n_slots", 0), ("n_slots", 24), ("n_arfcn", 6), ("d_row", None)):
        r = pkg.TrxGroupResult(); C.pointer(r)[0] = res
        setattr(r, field, v)
        assert L.trxsig_l1hop_result(hp.h, 0, C.byref(r), C.byref(out)) == EINVAL, field
    assert L.trxsig_l1hop_result(hp.h, HYPER, C.byref(res), C.byref(out)) == EINVAL
    assert L.trxsig_l1hop_result(hp.h, -1, C.byref(res), C.byref(out)) == EINVAL
    assert L.trxsig_l1hop_result(hp.h, 0, None, C.byref(out)) == EINVAL and L.trxsig_l1hop_result(hp.h, 0, C.byref(res), None) == EINVAL
    assert not out.d_row
    ctx.synchronize()
    assert np.array_equal(d.cpu().numpy(), src) and (y == 1).all()       # nothing was launched
    hp.bits(1, 5, 2, d)                                      # and good calls still go through
    hp.cells(1, 5, 2, x, 7 * 640, 640, y, 7 * 640, 640)
    hp.result(res, 5)
    ctx.synchronize()
    assert (d.cpu().numpy() != src).any() and (y.reshape(16, 7, 640, 2)[:, :, :624] == 0).all()
    hp.destroy()
