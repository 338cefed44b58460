"""GPU parity of the uplink L1 demultiplexer (trxsig_l1rx.h) against the literal model (tests/l1_demux_model.py): status,
frames, FER, closing FNs, the decoders' state bytes, the RACH list, RSSI / timing and SACCH power / TA, exactly.  Random plans
and streams (missing and invalid bursts, both wire settings, closed channels), chaining across the 5304 period and the
hyperframe wrap, the bad-input rules, a closed loop (encoders -> GMSK -> trxsig_trxgroup_pull -> decode, every payload, RA
and SACCH power / TA back, the model fed with trxsig_trxgroup_collect) and RSSI at the floor boundaries."""

import numpy as np
import pytest

import _pkg
import fec_stream_model as fsm
import l1_demux_model as ldm

pytestmark = pytest.mark.gpu
HYPER = ldm.HYPERFRAME


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


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Pull:
    """A trxsig_trxgroup_result built from tensors, and what trxsig_trxgroup_collect would report for it."""

    def __init__(self, pkg, rng, model, fn, F, p_drop=0.15, sps=4, phy=None, rach_bsic=None):
        """phy(rng, n_rows) -> (amp[n_rows, 2], toa[n_rows]) replaces the random amplitudes and TOAs; rach_bsic: access bursts
        that carry a random RA, every other one with this BSIC, at the RACH positions (else noise)."""
        A = model.A
        T = 8 * F
        bits = {}
        soft = np.zeros((T, A, 148), np.float32)
        for k in range(F):
            u = fn + k
            for tn in range(8):
                for a in range(A):
                    c = model.table[a][tn][(u % HYPER) % ldm.MAX_MODULUS]
                    if c is not None and c.cls == ldm.XCCH:        # XCCH blocks carry real L2 frames
                        key = (id(c), model.next_closing(c, u))
                        if key not in bits:
                            fr = rng.integers(0, 256, 23).astype(np.uint8)
                            bits[key] = model.p.fo.xcch_encode(fr, np.zeros(26, np.uint8)).reshape(4, 148)
                        soft[8 * k + tn, a] = fsm.soft_from_bits(rng, bits[key][c.m.reverse(u % HYPER) % 4], 0.3)
                    elif c is not None and c.cls == ldm.RACH and rach_bsic is not None:
                        soft[8 * k + tn, a] = rng.random(148).astype(np.float32)
                        e = rach_e36(model.p.fo, int(rng.integers(0, 256)), rach_bsic if (k + a) % 2 == 0 else rach_bsic ^ 0x2A)
                        soft[8 * k + tn, a, 49:85] = fsm.soft_from_bits(rng, e, 0.3)
                    else:
                        soft[8 * k + tn, a] = rng.random(148).astype(np.float32)
        present = rng.random((T, A)) >= p_drop
        n_rows = int(present.sum()) + 5
        perm = rng.permutation(n_rows)
        row = np.full((T, A), -1, np.int32)
        row[present] = perm[:int(present.sum())]
        rows = rng.random((n_rows, 160)).astype(np.float32)
        rows[row[present], :148] = soft[present]
        valid = (rng.random(n_rows) >= 0.1).astype(np.uint8) * pkg.F_DETECT
        if phy is None:
            amp = (rng.standard_normal((n_rows, 2)) * 3000).astype(np.float32)
            toa = (rng.standard_normal(n_rows) * 3).astype(np.float32)
        else:
            amp, toa = phy(rng, n_rows)
        self.t = dict(row=dev(row), valid=dev(valid), amp=dev(amp), toa=dev(toa), soft=dev(rows))
        self.res = pkg.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=n_rows, d_row=self.t["row"].data_ptr(),
                                      d_valid=self.t["valid"].data_ptr(), d_flags=None, d_amp=self.t["amp"].data_ptr(),
                                      d_toa=self.t["toa"].data_ptr(), d_avgpwr=None, d_threshold=None,
                                      d_soft=self.t["soft"].data_ptr(), soft_stride=160)
        ok = (row >= 0) & (valid[np.maximum(row, 0)] != 0)
        r = np.maximum(row, 0)
        a = amp[r]
        n2 = (a[..., 1] * a[..., 1] + a[..., 0] * a[..., 0]).astype(np.float32)
        absA = np.sqrt(n2.astype(np.float64)).astype(np.float32)
        rssi = np.floor(20.0 * np.log10(9450.0 / absA.astype(np.float64))).astype(np.int64)
        x = toa[r].astype(np.float64) * 256.0 / sps
        timing = (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)
        self.col = dict(valid=ok, soft=rows[r, :148], rssi=np.where(ok, rssi, 0), timing=np.where(ok, timing, 0))


def assert_same(g, m, what=""):
    for key in ("tch", "xcch"):
        mo = m[key]
        for gk, mk in (("status", "status"), ("fn", "fn"), ("rssi", "rssi"), ("timing", "timing")):
            assert np.array_equal(g[key + "_" + gk], mo[mk]), (what, key, gk, np.argwhere(g[key + "_" + gk] != mo[mk])[:5])
        assert np.array_equal(g[key + "_fer"].view(np.uint32), mo["fer"].view(np.uint32)), (what, key, "fer")
        assert np.array_equal(g[key], mo["frames"]), (what, key, "frames")
        assert np.array_equal(g[key + "_state"], mo["state"]), (what, key, "state")
    assert np.array_equal(g["facch"], m["tch"]["facch"]), (what, "facch")
    assert np.array_equal(g["ms_power"], m["xcch"]["power"]) and np.array_equal(g["ms_ta"], m["xcch"]["ta"]), (what, "power / TA")
    for k in ("fn", "arfcn", "rssi", "timing", "ok", "ra"):
        assert np.array_equal(g["rach"][k], m["rach"][k]), (what, "rach", k)


def random_plan(rng, A):
    comb = rng.choice(np.array([0, 1, 1, 7], np.uint8), (A, 8))
    comb[0, 0] = 5
    return comb


@pytest.mark.parametrize("wire", [True, False])
def test_random_plans_and_streams(pkg, ctx, prims, wire):
    rng = np.random.default_rng(300 + wire)
    A, F = 3, 104
    comb = random_plan(rng, A)
    model = ldm.Model(comb, bsic=rng.integers(0, 64), band=[900, 1800, 1900][wire], prims=prims)
    l1 = pkg.L1Rx(ctx, comb, model.bsic, model.band)
    assert [l1.channels(c) for c in (0, 1, 2)] == [len(model.ch[c]) for c in (0, 1, 2)]
    for cls in (0, 1):                                       # some channels closed
        for i in rng.choice(len(model.ch[cls]), max(1, len(model.ch[cls]) // 6), replace=False):
            l1.close(cls, int(i))
            model.ch[cls][i].active = False
    fn = int(rng.integers(0, 5000))
    for call in range(2):
        p = Pull(pkg, rng, model, fn, F)
        l1.decode(p.res, fn, wire=wire)
        g = l1.collect()
        m = model.decode(p.col, fn, wire=wire)
        assert_same(g, m, ("call", call))
        fn = (fn + F) % HYPER
        if call == 0:                                        # reopen one closed channel: FER reset, SACCH defaults
            for cls in (0, 1):
                c = next(i for i, ch in enumerate(model.ch[cls]) if not ch.active)
                l1.open(cls, c)
                model.ch[cls][c].open()
    st = m["xcch"]["status"]
    assert (st & fsm.TCH_GOOD).any() and (m["tch"]["status"] & fsm.DECODED).any()
    assert (m["xcch"]["power"] != 40).any() and len(m["rach"]["fn"]) > 0


@pytest.mark.parametrize("fn0", [5304 * 3 - 90, HYPER - 110])
def test_chaining_across_the_wraps(pkg, ctx, prims, fn0):
    rng = np.random.default_rng(fn0 % 1000)
    A, F = 2, 208
    comb = random_plan(rng, A)
    comb[1, 3] = 1
    chain_vs_whole(pkg, ctx, prims, rng, comb, fn0, F)


def chain_vs_whole(pkg, ctx, prims, rng, comb, fn0, F, n_cuts=4):
    """One decode of F frames from fn0 against the model, then the same pull decoded in n_cuts + 1 pieces at random frame
    cuts by a second L1Rx: every block, the final state and the RACH list equal the whole call's."""
    A = comb.shape[0]
    model = ldm.Model(comb, bsic=7, prims=prims)
    p = Pull(pkg, rng, model, fn0, F)
    whole = pkg.L1Rx(ctx, comb, 7)
    whole.decode(p.res, fn0)
    gw = whole.collect()
    assert_same(gw, model.decode(p.col, fn0), "whole")
    cuts = [0] + sorted(rng.choice(np.arange(1, F), n_cuts, replace=False).tolist()) + [F]
    part = pkg.L1Rx(ctx, comb, 7)
    blocks = {}
    rach = []
    for lo, hi in zip(cuts, cuts[1:]):
        import torch
        res = pkg.TrxGroupResult(n_slots=8 * (hi - lo), n_arfcn=A, n_rows=p.res.n_rows,
                                 d_row=p.t["row"][8 * lo:8 * hi].contiguous().data_ptr(), d_valid=p.res.d_valid, d_flags=None,
                                 d_amp=p.res.d_amp, d_toa=p.res.d_toa, d_avgpwr=None, d_threshold=None, d_soft=p.res.d_soft,
                                 soft_stride=160)
        keep = p.t["row"][8 * lo:8 * hi].contiguous()
        res.d_row = keep.data_ptr()
        part.decode(res, (fn0 + lo) % HYPER)
        g = part.collect()
        torch.cuda.synchronize()
        for key in ("tch", "xcch"):
            for s, b in zip(*np.nonzero(g[key + "_status"])):
                blocks[(key, s, int(g[key + "_fn"][s, b]))] = (g[key + "_status"][s, b], g[key][s, b].tobytes(),
                                                               g[key + "_fer"][s, b].tobytes())
        rach.append(g["rach"])
    want = {}
    for key in ("tch", "xcch"):
        for s, b in zip(*np.nonzero(gw[key + "_status"])):
            want[(key, s, int(gw[key + "_fn"][s, b]))] = (gw[key + "_status"][s, b], gw[key][s, b].tobytes(),
                                                          gw[key + "_fer"][s, b].tobytes())
    assert blocks == want
    for k in ("tch_state", "xcch_state", "tch_rssi", "tch_timing", "xcch_rssi", "xcch_timing", "ms_power", "ms_ta"):
        assert np.array_equal(g[k], gw[k]), k
    for k in ("fn", "ok", "ra", "rssi", "timing"):
        assert np.array_equal(np.concatenate([r[k] for r in rach]), gw["rach"][k]), k
    return whole, cuts, gw


def test_bad_inputs(pkg, ctx):
    import ctypes as C
    L, EINVAL = ctx.L, -1
    ok = np.zeros((2, 8), np.uint8); ok[0, 0] = 5; ok[1, :] = 7
    pkg.L1Rx(ctx, ok, 0).destroy()
    for bad in ([(1, 0, 5)], [(0, 1, 5)], [(0, 2, 4)], [(1, 3, 2)], [(0, 5, 9)]):
        comb = ok.copy()
        for a, tn, v in bad:
            comb[a, tn] = v
        h = C.c_void_p()
        assert L.trxsig_l1rx_create(C.byref(h), ctx.h, 2, comb.ctypes.data, 0, 900) == EINVAL, bad
    h = C.c_void_p()
    assert L.trxsig_l1rx_create(C.byref(h), ctx.h, 2, ok.ctypes.data, 64, 900) == EINVAL
    assert L.trxsig_l1rx_create(C.byref(h), ctx.h, 2, ok.ctypes.data, 1, 1000) == EINVAL
    assert L.trxsig_l1rx_create(C.byref(h), ctx.h, 2, None, 1, 900) == EINVAL
    l1 = pkg.L1Rx(ctx, ok, 3)
    rng = np.random.default_rng(5)
    model = ldm.Model(ok, 3)
    p = Pull(pkg, rng, model, 0, 2)
    out = pkg.L1RxOut()
    dec = lambda res, fn=0, o=out: L.trxsig_l1rx_decode(l1.h, res, fn, 1, o)
    assert dec(C.byref(p.res)) == 0
    for field, v in (("n_slots", 12), ("n_slots", 0), ("n_arfcn", 1), ("soft_stride", 100), ("d_row", None), ("n_rows", -1)):
        r = pkg.TrxGroupResult(); C.pointer(r)[0] = p.res
        setattr(r, field, v)
        assert dec(C.byref(r)) == EINVAL, field
    assert dec(C.byref(p.res), fn=HYPER) == EINVAL and dec(C.byref(p.res), fn=-1) == EINVAL
    assert dec(None) == EINVAL and dec(C.byref(p.res), o=None) == EINVAL
    assert L.trxsig_l1rx_open(l1.h, 2, 0) == EINVAL and L.trxsig_l1rx_close(l1.h, 1, 10 ** 6) == EINVAL
    assert L.trxsig_l1rx_channels(l1.h, 3) == EINVAL


def rach_e36(fo, ra, bsic):
    """A test-side RACH encoder (GSM 05.03 4.6, the inverse of RACHL1Decoder::writeLowSide): u[0..7] = RA with the LSB first
    (mD.LSB8MSB() then reads it MSB first), u[8..13] = ~(bsic ^ parity(u[0..7])), u[14..17] = 0 tail; 36 coded bits."""
    u = np.zeros(18, np.uint8)
    u[:8] = [(ra >> i) & 1 for i in range(8)]
    p = (~(bsic ^ fo.parity(fsm.fecbind.RACH_POLY, 6, u[:8]))) & 0x3F
    u[8:14] = [(p >> (5 - i)) & 1 for i in range(6)]
    e = fo.encode(u)
    r = fo.rach_decode(e.astype(np.float32))
    assert r["tail_ok"] and int(r["bsic"]) == bsic and int(r["ra"]) == ra
    return e


def test_closed_loop_through_a_group_pull(pkg, prims):
    """Speech / FACCH (trxsig_fec_tch_encode_batch), SDCCH / SACCH L2 frames with a physical header
    (trxsig_fec_xcch_encode_batch) and access bursts with the right and a wrong BSIC, each at its channel's uplink frames ->
    GMSK -> trxsig_trxgroup_pull with the plan's CMD SETSLOT -> trxsig_l1rx_decode.  Every payload, RA and SACCH power / TA
    comes back, and the result equals the model fed with trxsig_trxgroup_collect's output."""
    import torch
    from openbts_ttsou_amd import synth
    sps, tsc, A, F, fn0, bsic = 4, 3, 2, 208, 26 * 40, 21
    rng = np.random.default_rng(77)
    comb = np.zeros((A, 8), np.uint8)
    comb[0, :3] = [5, 1, 7]; comb[0, 4] = 1; comb[1, :2] = [1, 7]
    model = ldm.Model(comb, bsic, band=1800, prims=prims)
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    T = 8 * F
    chans = {cls: model.ch[cls] for cls in (ldm.TCH, ldm.XCCH, ldm.RACH)}
    # TCH: the channel's j-th burst of the window is burst j of its encoded stream (fn0 % 26 == 0: the first one has B = 0)
    nt, n = len(chans[ldm.TCH]), F * 24 // 104
    kind = np.where(rng.random((nt, n)) < 0.25, pkg.TCH_FACCH, pkg.TCH_SPEECH).astype(np.uint8)
    pl = rng.integers(0, 256, (nt, n, 33)).astype(np.uint8); pl[:, :, 32] &= 0xF0
    tb = torch.zeros(nt, n, 4, 148, dtype=torch.uint8, device="cuda")
    ctx.fec_tch_encode(dev(kind), dev(pl), dev(np.full(nt, tsc, np.uint8)), torch.zeros(nt, 32, dtype=torch.uint8, device="cuda"), tb)
    tbits = tb.cpu().numpy().reshape(nt, 4 * n, 148)
    # XCCH blocks keyed by (channel, closing frame); RACH bursts by frame
    cells, xkeys = {}, []
    tcount = [0] * nt
    rach_sent = {}
    for k in range(F):
        u = fn0 + k
        for tn in range(8):
            for a in range(A):
                c = model.table[a][tn][u % ldm.MAX_MODULUS]
                if c is None:
                    continue
                if c.cls == ldm.TCH:
                    i = chans[ldm.TCH].index(c)
                    cells[(8 * k + tn, a)] = ("t", i, tcount[i]); tcount[i] += 1
                elif c.cls == ldm.XCCH:
                    key = (chans[ldm.XCCH].index(c), model.next_closing(c, u))
                    if key not in xkeys:
                        xkeys.append(key)
                    cells[(8 * k + tn, a)] = ("x", xkeys.index(key), c.m.reverse(u) % 4)
                else:
                    ra, good = int(rng.integers(0, 256)), len(rach_sent) % 2 == 0
                    rach_sent[u] = (ra, good)
                    cells[(8 * k + tn, a)] = ("r", rach_e36(prims.fo, ra, bsic if good else bsic ^ 0x15))
    xfr = rng.integers(0, 256, (len(xkeys), 23)).astype(np.uint8)
    xb = torch.zeros(len(xkeys) * 4, 148, dtype=torch.uint8, device="cuda")
    ctx.fec_xcch_encode(dev(xfr), len(xkeys), tsc, xb)
    xbits = xb.cpu().numpy().reshape(len(xkeys), 4, 148)
    keys = sorted(cells)
    bb = np.zeros((len(keys), 148), np.uint8)
    for i, key in enumerate(keys):
        v = cells[key]
        if v[0] == "t":
            bb[i] = tbits[v[1], v[2]]
        elif v[0] == "x":
            bb[i] = xbits[v[1], v[2]]
        else:
            bb[i] = synth.rach_bits(rng, 1)[0]
            bb[i, 49:85] = v[1]
    xs, offs, lens, _ = synth.bursts_from_bits(bb, sps, seed=78, sigmas=(0.0, 0.02), max_delay=0.5)
    cell = 160 * sps
    x = np.zeros((T, A, cell), np.complex64)
    for i, (t, a) in enumerate(keys):
        nsmp = (156 + (t % 8 % 4 == 0)) * sps
        v = xs[offs[i]:offs[i] + lens[i]][:nsmp]
        x[t, a, :len(v)] = v
    grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn0, 0))
    for a in range(A):
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % tsc] + \
                   ["CMD SETSLOT %d %d" % (tn, comb[a, tn]) for tn in range(8)] + ["CMD POWERON"]:
            grp.control(a, cmd)
    dx = torch.from_numpy(x.view(np.float32).reshape(-1)).to("cuda:0")
    res = grp.pull(dx.data_ptr(), A * cell, cell, fn0, 0, T)
    grp.sync()
    l1 = pkg.L1Rx(ctx, comb, bsic, 1800)
    l1.decode(res, fn0)
    g = l1.collect()
    col = grp.collect()
    assert all(col["valid"][t, a] for (t, a) in keys), "a clean burst was not detected"
    m = model.decode(col, fn0)
    assert_same(g, m, "closed loop")
    # every payload back: TCH stream block b carries encoded block b - 1
    st = g["tch_status"]
    for s in range(nt):
        for b in range(1, n):
            if kind[s, b - 1] == pkg.TCH_SPEECH:
                assert st[s, b] == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(g["tch"][s, b], pl[s, b - 1]), (s, b)
            else:
                assert st[s, b] & fsm.FACCH_OK and np.array_equal(g["facch"][s, b], pl[s, b - 1, :23]), (s, b)
    # XCCH: every block whose four bursts lie in the window decodes to its frame; SACCH power / TA from the last good one
    complete = [(ci, f) for ci, f in xkeys if sum(model.next_closing(chans[ldm.XCCH][ci], u) == f for u in range(fn0, fn0 + F)
                                                  if chans[ldm.XCCH][ci].m.reverse(u) >= 0) == 4]
    assert len(complete) > 40
    power, ta = {}, {}
    for ci, f in complete:
        b = list(g["xcch_fn"][ci]).index(f % HYPER)
        fr = xfr[xkeys.index((ci, f))]
        assert g["xcch_status"][ci, b] == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(g["xcch"][ci, b], fr), (ci, f)
        if chans[ldm.XCCH][ci].sacch and (ci not in power or f > power[ci][0]):
            power[ci] = (f, ldm.POWER[1800][fr[0] & 31])
            if fr[1] & 127 < 64:
                ta[ci] = (f, fr[1] & 127)
    assert len(power) >= 4
    for ci, (f, p) in power.items():
        assert g["ms_power"][ci] == p
    for ci, (f, t) in ta.items():
        assert g["ms_ta"][ci] == t
    # access bursts: all listed in FN order, RA back where the BSIC is the cell's, refused where it is not
    r = g["rach"]
    assert list(r["fn"]) == sorted(u % HYPER for u in rach_sent) and (r["arfcn"] == 0).all()
    for f, ok, ra in zip(r["fn"], r["ok"], r["ra"]):
        want_ra, good = rach_sent[int(f)]
        assert ok == good and ra == (want_ra if good else 0), f
    assert r["ok"].any() and not r["ok"].all()
    l1.destroy(); grp.close(); ctx.close()


def test_rssi_at_the_floor_boundaries(pkg, ctx):
    """Amplitudes where 20 log10(9450 / |A|) is an integer (|A| = 9450 / 10^k), one float ulp to either side, and small |A|
    whose RSSI wraps through the datagram's signed byte: the device's per-channel RSSI equals trxsig_trxgroup_collect's
    formula evaluated with the C library's log10 (Transceiver.cpp:400), then the wire rule."""
    import math
    comb = np.ones((4, 8), np.uint8)
    l1 = pkg.L1Rx(ctx, comb, 0)
    n = l1.channels(pkg.L1_TCH)
    base = [9450.0, 945.0, 94.5, 9.45, 0.945, 0.0945, 94500.0, 945000.0, 1e-3, 2e-4, 5e-5, 3.0e-5]
    mags = []
    for v in base:
        f = np.float32(v)
        mags += [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(0))]
    mags = np.array(mags[:n], np.float32)
    assert len(mags) == n == 32
    # one frame (FN 0, a traffic frame on every slot): channel c = 8a + tn gets the burst of slot tn, ARFCN a
    row = np.arange(8 * 4, dtype=np.int32).reshape(4, 8).T.copy()          # [slot tn][arfcn a] -> row 8a + tn
    amp = np.zeros((n, 2), np.float32); amp[:, 0] = mags
    t = dict(row=dev(row), valid=dev(np.full(n, pkg.F_DETECT, np.uint8)), amp=dev(amp), toa=dev(np.zeros(n, np.float32)),
             soft=dev(np.full((n, 148), 0.5, np.float32)))
    res = pkg.TrxGroupResult(n_slots=8, n_arfcn=4, n_rows=n, d_row=t["row"].data_ptr(), d_valid=t["valid"].data_ptr(), d_flags=None,
                             d_amp=t["amp"].data_ptr(), d_toa=t["toa"].data_ptr(), d_avgpwr=None, d_threshold=None,
                             d_soft=t["soft"].data_ptr(), soft_stride=148)
    l1.decode(res, 0)
    g = l1.collect(state=False)
    for c in range(n):
        a = float(np.float32(np.sqrt(np.float64(np.float32(mags[c] * mags[c] + np.float32(0.0))))))
        db = math.floor(20.0 * math.log10(9450.0 / a))
        assert g["tch_rssi"][c] == ldm.wire_phy(db, 0)[0], (c, mags[c], db)
    assert (g["tch_rssi"] > 0).any() and (g["tch_rssi"] < 0).any()
    l1.destroy()


# ---- production scale: the plan tools/l1rx_bench.py times, a RACH list past one k_l1rx_finish block, the wraps at that
# scale, and RSSI / TOA values that wrap through the datagram's signed byte and int16 ----
def big_plan(rng, A):
    comb = rng.choice(np.array([0, 1, 1, 7], np.uint8), (A, 8))
    comb[0, 0] = 5
    return comb


@pytest.mark.timeout(900)
@pytest.mark.parametrize("wire", [True, False])
def test_production_plan_over_consecutive_calls(pkg, ctx, prims, wire):
    """128 ARFCNs x 104 frames (C0T0 combination V, the rest a mix of I, VII and unused slots), some channels closed and one
    reopened between calls, three consecutive calls."""
    rng = np.random.default_rng(800 + wire)
    A, F = 128, 104
    comb = big_plan(rng, A)
    model = ldm.Model(comb, bsic=int(rng.integers(0, 64)), band=1800, prims=prims)
    l1 = pkg.L1Rx(ctx, comb, model.bsic, model.band)
    closed = {}
    for cls in (0, 1):
        closed[cls] = rng.choice(len(model.ch[cls]), len(model.ch[cls]) // 10, replace=False)
        for i in closed[cls]:
            l1.close(cls, int(i))
            model.ch[cls][i].active = False
    fn = int(rng.integers(0, HYPER - 3 * F))
    for call in range(3):
        p = Pull(pkg, rng, model, fn, F, rach_bsic=model.bsic)
        l1.decode(p.res, fn, wire=wire)
        g = l1.collect()
        m = model.decode(p.col, fn, wire=wire)
        assert_same(g, m, ("call", call))
        if call == 0:
            for cls in (0, 1):
                i = int(closed[cls][0])
                l1.open(cls, i)
                model.ch[cls][i].open()
        fn += F
    o = l1.out
    assert o.n_xcch > 256 and o.n_tch > 256 and o.n_xcch == len(model.ch[ldm.XCCH])
    st = m["xcch"]["status"]
    assert (st & fsm.TCH_GOOD).any() and (m["tch"]["status"] & fsm.DECODED).any() and m["rach"]["ok"].any()
    assert (m["xcch"]["power"] != 40).any()
    l1.destroy()


@pytest.mark.timeout(600)
def test_rach_list_past_one_finish_block(pkg, ctx, prims):
    """680 frames: the C0T0 RACH positions number more than 256 (rach_cap > 256, so k_l1rx_demux builds its list over many
    64-position chunks and k_l1rx_finish runs several blocks for it); access bursts at most of them, half with the cell's
    BSIC."""
    rng = np.random.default_rng(900)
    A, F, bsic = 2, 680, 45
    comb = big_plan(rng, A)
    model = ldm.Model(comb, bsic=bsic, prims=prims)
    l1 = pkg.L1Rx(ctx, comb, bsic)
    fn = 5304 - 77
    for call in range(2):
        p = Pull(pkg, rng, model, fn, F, p_drop=0.1, rach_bsic=bsic)
        l1.decode(p.res, fn)
        g = l1.collect()
        m = model.decode(p.col, fn)
        assert_same(g, m, ("call", call))
        assert l1.out.rach_cap > 256 and len(m["rach"]["fn"]) > 256
        assert m["rach"]["ok"].sum() > 100 and not m["rach"]["ok"].all()
        fn += F
    l1.destroy()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fn0", [5304 * 7 - 61, HYPER - 53])
def test_chaining_across_the_wraps_at_scale(pkg, ctx, prims, fn0):
    """128 ARFCNs x 104 frames across the 5304 period / the hyperframe wrap, whole against the model and against six pieces cut
    at random frames (not block-aligned)."""
    rng = np.random.default_rng(fn0 % 997)
    comb = big_plan(rng, 128)
    whole, cuts, gw = chain_vs_whole(pkg, ctx, prims, rng, comb, fn0, 104, n_cuts=5)
    wrap = (fn0 // 5304 + 1) * 5304                          # the next 5304 boundary (HYPER is one of them)
    assert any((fn0 + lo) < wrap < (fn0 + hi) or fn0 + lo == wrap for lo, hi in zip(cuts, cuts[1:]))
    assert any(c % 4 for c in cuts) and whole.out.n_xcch > 256


def wild_phy(rng, n):
    """amplitudes from 1e-18 to 1e18 (20 log10(9450 / |A|) from about -281 to 439, inside and outside the signed byte),
    TOAs whose round(toa * 256 / sps) leaves int16 (and sits on its boundary: 32767.5 -> 32768 wraps)"""
    mag = np.where(rng.random(n) < 0.2, rng.standard_normal(n) * 3000, 10.0 ** rng.uniform(-18, 18, n))
    ph = rng.uniform(0.2, 1.37, n) + np.pi / 2 * rng.integers(0, 4, n)   # both components >= 0.2 |A|: no subnormal square
    amp = np.stack([mag * np.cos(ph), mag * np.sin(ph)], 1).astype(np.float32)
    x = np.where(rng.random(n) < 0.5, rng.standard_normal(n) * 3 * 64, rng.uniform(-4e7, 4e7, n))
    edge = np.array([32767.4, 32767.5, 32768.0, 32768.5, -32768.4, -32768.5, -32769.0, 65535.5, 65536.5, -65536.5, 127.5, -128.5])
    x[:len(edge) * 20] = np.tile(edge, 20)
    toa = (x / 64.0).astype(np.float32)                       # sps = 4: round(toa * 64)
    return amp, toa


def test_rssi_and_toa_wrap_like_the_datagram(pkg, ctx, prims):
    """RSSI / timing values outside the datagram's ranges on every channel kind (TCH and XCCH per-channel values, RACH list):
    equal the model, whose narrowing tests/test_l1_demux_model.py checks against the reference's byte path."""
    rng = np.random.default_rng(1000)
    A, F = 4, 104
    comb = big_plan(rng, A)
    model = ldm.Model(comb, bsic=3, prims=prims)
    l1 = pkg.L1Rx(ctx, comb, 3)
    fn = 1234
    wrapped_db = wrapped_t = 0
    for call in range(3):
        p = Pull(pkg, rng, model, fn, F, phy=wild_phy, rach_bsic=3)
        l1.decode(p.res, fn)
        g = l1.collect()
        m = model.decode(p.col, fn)
        assert_same(g, m, ("call", call))
        routed = np.zeros_like(p.col["valid"])
        for k in range(F):
            for tn in range(8):
                for a in range(A):
                    routed[8 * k + tn, a] = model.table[a][tn][((fn + k) % HYPER) % ldm.MAX_MODULUS] is not None
        on = p.col["valid"] & routed
        db, tt = p.col["rssi"][on], p.col["timing"][on]
        wrapped_db += int(((db > 127) | (db < -128)).sum())
        wrapped_t += int(((tt > 32767) | (tt < -32768)).sum())
        assert (db > 127).any() and (db < -128).any() and (tt > 32767).any() and (tt < -32768).any()
        fn += F
    r = m["rach"]
    assert wrapped_db > 100 and wrapped_t > 100 and len(r["fn"]) > 0
    l1.destroy()
