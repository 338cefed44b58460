"""GPU parity of the packet data channel object (include/trxsig_l1pdch.h) against tests/l1_pdch_model.py, byte for byte: the
encoder's grid, what bytes and channel records (pending bursts, USF ring) over call sizes 1 / 4 / 13 / 52 / 110 from fn 0, 9 and
across the hyperframe; splits equal to the whole; the overlay onto trxsig_l1tx's grid and onto caller arrays with canaries; the
decoder's every output and record on clean and noisy rows, missing and invalid bursts, NaN and infinities, both wire settings,
every cs_force, splits; the grant; a closed loop on the card through a Transceiver group; and, last, the refusals.

Shapes: 3 ARFCNs; PDCH on (0, 1), (0, 7), (2, 0), (2, 4) -- TN 0 and TN 4 are the 157-symbol slots -- among combinations 5 / 7 / 1,
which the object ignores; the schemes are mixed inside every channel."""
import numpy as np
import pytest

import _pkg
import fecbind
import fectxbind
import l1_pdch_model as lp

pytestmark = pytest.mark.gpu

HYPER = lp.HYPER
COMB = np.array([[5, 13, 1, 7, 0, 0, 1, 13], [1, 7, 0, 0, 1, 1, 7, 0], [13, 1, 7, 0, 13, 1, 0, 0]], np.uint8)
BSIC = 0x2D
SIZES = [1, 4, 13, 52, 110]
FNS = [0, 9, HYPER - 30]
CANARY, PAD = 0xA5, 64
SPLITS = [(1,), (12, 13), (3, 4, 5, 25, 26), (38, 39, 51, 52, 64), (90, 91, 104), (1, 3, 4, 5, 12, 13, 25, 26, 38, 39, 51, 52, 64, 90, 91, 104)]


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
def o():
    return fecbind.FecOracle()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def model(o, direction, comb=COMB):
    return lp.Model(comb, BSIC, direction, o, fectxbind.TSC_BITS)


def gpu_encode(obj, fn, F, ins, **kw):
    return obj.encode(fn % HYPER, F, dev(ins["kind"]), dev(ins["cs"]), dev(ins["payload"]), dev(ins["pt_kind"]), dev(ins["pt_payload"]), **kw)


def same_states(obj, m, what):
    st = obj.states()
    for cls in (lp.PDTCH, lp.PTCCH):
        g, w = st[cls], m.state(cls)
        assert g.shape == w.shape and np.array_equal(g, w), (what, cls, np.argwhere(g != w)[:6])


@pytest.fixture(scope="module")
def whole(o):
    """fn -> (inputs of the 110-frame call, the DOWN model after it, its grid and what): computed once, read by several tests."""
    cache = {}

    def get(fn):
        if fn not in cache:
            m = model(o, lp.DOWN)
            ins = lp.random_inputs(np.random.default_rng(fn % 997), m, fn, 110)
            bits, what = m.encode(fn, 110, **ins)
            for a in list(ins.values()) + [bits, what]:
                a.flags.writeable = False
            cache[fn] = (ins, m, bits, what)
        return cache[fn]
    return get


# ---- encode ----
@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("direction", [lp.DOWN, lp.UP])
def test_encoder_equals_model(pkg, ctx, o, fn, direction):
    """The five call sizes one after the other from fn: grid, what and the records (pending bursts, ring) after every call."""
    m, obj = model(o, direction), pkg.L1Pdch(ctx, COMB, BSIC, direction)
    assert [obj.channels(c) for c in (0, 1)] == [4, 4 if direction == lp.DOWN else 0]
    assert [obj.channel(0, i) for i in range(4)] == [(0, 1), (0, 7), (2, 0), (2, 4)]
    assert np.array_equal(obj.circuit_plan(), lp.circuit_plan(COMB)) and not (obj.circuit_plan() == 13).any()
    rng = np.random.default_rng(fn % 1000 + direction)
    f0, sent_any, idle_any = fn, False, False
    for F in SIZES:
        assert obj.grid(f0 % HYPER, F) == m.grid(f0, F)
        ins = lp.random_inputs(rng, m, f0, F)
        bits, what = m.encode(f0, F, **ins)
        gpu_encode(obj, f0, F, ins)
        g = obj.collect()
        assert np.array_equal(g["what"], what), (F, np.argwhere(g["what"] != what)[:6])
        assert np.array_equal(g["bits"], bits), (F, np.argwhere((g["bits"] != bits).any(axis=2))[:6])
        same_states(obj, m, F)
        not_sent = (ins["kind"] != 1) | (ins["cs"] > 3)
        sent_any |= bool((~not_sent).any()); idle_any |= bool(not_sent.any())
        f0 += F
    assert sent_any and idle_any                             # a cs of 4 / 255 and a kind of 0 / 2 sent nothing: the model's zeros
    assert (m.st[0]["ring"] >= 0).any() == (direction == lp.DOWN)
    obj.destroy()


@pytest.mark.parametrize("fn", FNS)
def test_encoder_splits_equal_the_whole(pkg, ctx, o, whole, fn):
    ins, m, bits, what = whole(fn)
    for cuts in [()] + SPLITS:
        obj = pkg.L1Pdch(ctx, COMB, BSIC, lp.DOWN)
        edges = [0] + list(cuts) + [110]
        gb, gw = [], []
        for a, b in zip(edges[:-1], edges[1:]):
            gpu_encode(obj, fn + a, b - a, lp.slice_inputs(m, ins, fn, 110, fn + a, fn + b))
            g = obj.collect()
            gb.append(g["bits"]); gw.append(g["what"])
        assert np.array_equal(np.concatenate(gw, axis=1), what) and np.array_equal(np.concatenate(gb, axis=1), bits), cuts
        same_states(obj, m, cuts)
        obj.destroy()


def test_overlay_onto_l1tx_and_caller_arrays(pkg, ctx, o):
    """onto trxsig_l1tx's last grid (the circuit plan's encode), and onto caller arrays, aligned and not, with canaries behind
    both: every slot the model does not write is the copy taken before, the written ones are the model's."""
    import torch
    fn, F = 9, 52
    m, obj = model(o, lp.DOWN), pkg.L1Pdch(ctx, COMB, BSIC, lp.DOWN)
    tx = pkg.L1Tx(ctx, obj.circuit_plan(), BSIC)
    nb = tx.grid(fn, F)
    rng = np.random.default_rng(12)
    z = lambda n, b, w: dev(np.zeros((n, b, w), np.uint8)) if w else dev(np.zeros((n, b), np.uint8))
    nt, nx, nc = (tx.channels(c) for c in (pkg.L1_TCH, pkg.L1_XCCH, pkg.L1_CCCH))
    xk = dev((rng.random((nx, nb[1])) < 0.7).astype(np.uint8))
    xp = dev(rng.integers(0, 256, (nx, nb[1], 23)).astype(np.uint8))
    tx.encode(fn, F, z(nt, nb[0], 0), dev(rng.integers(0, 256, (nt, nb[0], 33)).astype(np.uint8)), xk, xp, z(nc, nb[2], 0), z(nc, nb[2], 23))
    before = tx.collect(state=False)
    assert (before["what"] != 0).sum() > 300
    pdch = np.repeat((COMB == 13)[:, None, :], F, axis=1).reshape(3, 8 * F)
    assert not before["what"][pdch].any() and not before["bits"][pdch].any()     # the circuit plan leaves the packet slots empty
    ins = lp.random_inputs(rng, m, fn, F)
    bits, what = m.encode(fn, F, onto=(before["bits"], before["what"]), **ins)
    gpu_encode(obj, fn, F, ins, bits_onto=tx.out.d_bits, what_onto=tx.out.d_what)
    after = tx.collect(state=False)
    assert np.array_equal(after["what"], what) and np.array_equal(after["bits"], bits)
    wrote = what != before["what"]
    assert wrote.sum() > 100 and (what[wrote] == pkg.L1TX_PDCH).all() and np.array_equal(after["bits"][~wrote], before["bits"][~wrote])
    # caller arrays: the same call from fresh records, onto padded copies; misaligned by one byte for the byte-store form
    nbits, nwhat = 3 * 8 * F * 148, 3 * 8 * F
    for mis in (0, 1):
        obj2 = pkg.L1Pdch(ctx, COMB, BSIC, lp.DOWN)
        db = torch.full((mis + nbits + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        dw = torch.full((mis + nwhat + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        db[mis:mis + nbits] = dev(before["bits"].reshape(-1)); dw[mis:mis + nwhat] = dev(before["what"].reshape(-1))
        gpu_encode(obj2, fn, F, ins, bits_onto=db[mis:], what_onto=dw[mis:])
        ctx.synchronize()
        hb, hw = db.cpu().numpy(), dw.cpu().numpy()
        assert (hb[:mis] == CANARY).all() and (hb[mis + nbits:] == CANARY).all() and (hw[:mis] == CANARY).all() and (hw[mis + nwhat:] == CANARY).all()
        assert np.array_equal(hb[mis:mis + nbits].reshape(bits.shape), bits) and np.array_equal(hw[mis:mis + nwhat].reshape(what.shape), what)
        obj2.destroy()
    tx.destroy(); obj.destroy()


# ---- decode ----
class Pull:
    """A trxsig_trxgroup_result built from tensors for the bursts soft[T][A][148] at the slots `present`, and what
    trxsig_trxgroup_collect would report for it (as tests/test_gpu_l1rx.py builds one)."""

    def __init__(self, pkg, rng, soft, present, p_invalid=0.1, sps=4):
        T, A = present.shape
        n = int(present.sum())
        n_rows = n + 5
        row = np.full((T, A), -1, np.int32)
        row[present] = rng.permutation(n_rows)[:n]
        rows = rng.random((n_rows, 160)).astype(np.float32)   # a stride above 148; rows nobody uses hold noise
        rows[row[present], :148] = soft[present]
        valid = (rng.random(n_rows) >= p_invalid).astype(np.uint8) * pkg.F_DETECT
        amp = (rng.standard_normal((n_rows, 2)) * 3000).astype(np.float32)
        toa = (rng.standard_normal(n_rows) * 3).astype(np.float32)
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

    def part(self, pkg, k0, k1):
        """frames [k0, k1) of the pull as a result of their own (the same rows) and its collect"""
        A = self.col["valid"].shape[1]
        row = self.t["row"][8 * k0:8 * k1].contiguous()
        res = pkg.TrxGroupResult.from_buffer_copy(self.res)
        res.n_slots, res.d_row = 8 * (k1 - k0), row.data_ptr()
        return res, {k: v[8 * k0:8 * k1] for k, v in self.col.items()}, row


def soft_grid(rng, bits, what, sigma, clip, p_drop=0.12, hostile=False):
    """[T][A][148] soft values of an encoder's grid, where they are present: dropped slots have d_row = -1; slots nobody wrote
    carry noise (the demultiplexer must not take them: frames 12 / 25 / 38 / 51, other combinations' slots)."""
    T, A = what.shape[1], what.shape[0]
    v = bits.transpose(1, 0, 2).astype(np.float32)
    if sigma:
        v = (v + rng.normal(0, sigma, v.shape)).astype(np.float32)
    if clip:
        v = np.clip(v, 0, 1)
    noise = rng.random(v.shape).astype(np.float32)
    w = what.T != 0
    v[~w] = noise[~w]
    if hostile:                                              # NaN values and rows, infinities (no UDP hop: undefined for them)
        idx = np.argwhere(w)
        for i, (t, a) in enumerate(idx[rng.permutation(len(idx))[:24]]):
            if i % 3 == 0:
                v[t, a, rng.integers(0, 148, 3)] = np.nan
            elif i % 3 == 1:
                v[t, a] = np.nan
            else:
                v[t, a] = np.where(rng.random(148) < 0.5, np.inf, -np.inf)
    present = rng.random((T, A)) >= p_drop
    return v, present


def slack_canaries(pkg, ctx, dec, fill):
    """The bytes between the end of every decode output and the next 256-byte boundary (each output is a region of its own in
    the object's workspace): filled with the canary, or checked."""
    for name, n, nb, np_ in (("pdtch", dec.n_pdtch, dec.nb_pdtch, 54), ("ptcch", dec.n_ptcch, dec.nb_ptcch, 23)):
        for f, width in (("payload", np_), ("cs", 1), ("cs_dist", 1), ("ok", 1), ("usf", 1), ("nb", 1), ("granted", 1), ("fn", 4)):
            used = n * nb * width
            room = -used % 256
            ptr = getattr(dec, "d_%s_%s" % (name, f))
            if not ptr or not used or not room:
                continue
            t = pkg._dev_tensor(ctx, ptr + used, (room,), "|u1")
            if fill:
                t.fill_(CANARY)
            else:
                assert bool((t == CANARY).all()), ("written past the end of an output", name, f)


def same_decode(g, m, what):
    for name in ("pdtch", "ptcch"):
        for k in ("nb", "fn", "cs", "cs_dist", "ok", "usf", "granted", "payload", "rssi", "timing"):
            assert g[name][k].shape == m[name][k].shape, (what, name, k, g[name][k].shape, m[name][k].shape)
            assert np.array_equal(g[name][k], m[name][k]), (what, name, k, np.argwhere(g[name][k] != m[name][k])[:6])


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("wire,sigma", [(True, 0.0), (True, 0.25), (True, 0.45), (False, 0.0), (False, 0.25), (False, 0.45)])
def test_decoder_equals_model(pkg, ctx, o, whole, fn, wire, sigma):
    """The whole call's bits as soft rows, decoded in the five call sizes one after the other, with a cs_force per call: every output and the records after every call.  d_row = -1 and d_valid = 0 remove bursts; the slots
    and frames no packet channel owns hold noise; without the UDP hop some rows are NaN or infinite."""
    ins, mtx, bits, what = whole(fn)
    rng = np.random.default_rng(int(1000 * sigma) + wire + fn % 89)
    soft, present = soft_grid(rng, bits, what, sigma, clip=wire, hostile=not wire)
    pull = Pull(pkg, rng, soft, present)
    m, obj = model(o, lp.DOWN), pkg.L1Pdch(ctx, COMB, BSIC, lp.DOWN)
    k0 = 0
    seen = set()
    with np.errstate(invalid="ignore"):
        for F, force in zip(SIZES, (-1, 0, 1, 2, 3)):
            F = min(F, 110 - k0)                             # (the last call takes what is left of the 110 frames)
            res, col, keep = pull.part(pkg, k0, k0 + F)
            obj.decode(res, (fn + k0) % HYPER, wire=wire, cs_force=force)
            g = obj.collect_decode()
            want = m.decode(col, fn + k0, wire=wire, cs_force=force)
            same_decode(g, want, (F, force))
            same_states(obj, m, (F, force))
            seen |= set(np.unique(want["pdtch"]["nb"]))
            k0 += F
    assert seen >= {0, 1, 3, 4}
    obj.destroy()


def test_outputs_stay_inside_their_regions(pkg, ctx, o, whole):
    """Canaries behind every decode output: the same call twice (the workspace does not move), the slack behind each output
    filled in between."""
    ins, mtx, bits, what = whole(9)
    rng = np.random.default_rng(8)
    soft, present = soft_grid(rng, bits, what, 0.2, clip=True)
    pull = Pull(pkg, rng, soft, present)
    obj = pkg.L1Pdch(ctx, COMB, BSIC, lp.DOWN)
    for F in (13, 52, 110):
        res, col, keep = pull.part(pkg, 0, F)
        dec = obj.decode(res, 9)
        ctx.synchronize()
        slack_canaries(pkg, ctx, dec, fill=True)
        again = obj.decode(res, 9)
        ctx.synchronize()
        assert all(getattr(again, f) == getattr(dec, f) for f, _ in dec._fields_)
        slack_canaries(pkg, ctx, again, fill=False)
    obj.destroy()


@pytest.mark.parametrize("fn", FNS)
def test_decoder_splits_equal_the_whole(pkg, ctx, o, whole, fn):
    """Block for block by closing FN, and the records, for wire_quantise 1 and 0."""
    ins, mtx, bits, what = whole(fn)
    rng = np.random.default_rng(fn % 77)
    soft, present = soft_grid(rng, bits, what, 0.3, clip=True)
    pull = Pull(pkg, rng, soft, present)

    def closed(g):
        out = {}
        for name in ("pdtch", "ptcch"):
            r = g[name]
            for ci, j in zip(*np.nonzero(r["fn"] >= 0)):
                out[(name, int(ci), int(r["fn"][ci, j]))] = tuple(np.asarray(r[k][ci, j]).tobytes() for k in
                                                                 ("payload", "cs", "cs_dist", "ok", "usf", "nb", "granted"))
        return out

    for wire in (True, False):
        ref = None
        for cuts in [()] + SPLITS:
            obj = pkg.L1Pdch(ctx, COMB, BSIC, lp.DOWN)
            edges = [0] + list(cuts) + [110]
            blocks = {}
            for a, b in zip(edges[:-1], edges[1:]):
                res, col, keep = pull.part(pkg, a, b)
                obj.decode(res, (fn + a) % HYPER, wire=wire)
                got = closed(obj.collect_decode())
                assert not set(got) & set(blocks)
                blocks.update(got)
            g = obj.collect_decode()
            final = (blocks, obj.states(), g["pdtch"]["rssi"], g["pdtch"]["timing"], g["ptcch"]["rssi"], g["ptcch"]["timing"])
            if ref is None:
                ref = final
                assert len(blocks) >= 4 * 25
            else:
                assert final[0] == ref[0], cuts
                for cls in (0, 1):
                    assert np.array_equal(final[1][cls], ref[1][cls]), (cuts, cls)
                assert all(np.array_equal(x, y) for x, y in zip(final[2:], ref[2:])), cuts
            obj.destroy()


def test_grant(pkg, ctx, o, whole):
    """With the DOWN sibling that encoded the same frames the grant equals the model's; a NULL sibling gives 255; a sibling with
    another plan is refused."""
    fn = 9
    ins, mtx, bits, what = whole(fn)
    down = pkg.L1Pdch(ctx, COMB, BSIC, lp.DOWN)
    gpu_encode(down, fn, 110, ins)
    same_states(down, mtx, "sibling")
    rng = np.random.default_rng(21)
    mu = model(o, lp.UP)
    uins = lp.random_inputs(rng, mu, fn, 110)
    ubits, uwhat = mu.encode(fn, 110, **uins)
    soft, present = soft_grid(rng, ubits, uwhat, 0.1, clip=True)
    pull = Pull(pkg, rng, soft, present)
    up, mrx = pkg.L1Pdch(ctx, COMB, BSIC, lp.UP), model(o, lp.UP)
    up.decode(pull.res, fn, sibling=down)
    g = up.collect_decode()
    want = mrx.decode(pull.col, fn, sibling=mtx)
    same_decode(g, want, "grant")
    gr = want["pdtch"]["granted"]
    assert (gr != 255).sum() > 40 and (gr == 255).sum() > 4 and g["ptcch"]["granted"].size == 0
    up.decode(pull.res, fn + 0, sibling=None)
    assert (up.collect_decode()["pdtch"]["granted"] == 255).all()
    other = COMB.copy(); other[1, 3] = 13
    sib2 = pkg.L1Pdch(ctx, other, BSIC, lp.DOWN)
    with pytest.raises(pkg.TrxSigError, match="sibling"):
        up.decode(pull.res, fn, sibling=sib2)
    for x in (down, up, sib2):
        x.destroy()


def test_closed_loop_on_the_card(pkg, ctx, o):
    """An UP object as the handset encodes 30 noise-free frames of mixed schemes -> trxsig_modulate_batch -> slot cells -> a
    Transceiver group with SETSLOT type 1 on the packet slots -> pull -> decode on a second UP object: every block sent comes back
    ok with its payload, scheme and USF, every block not sent has nb == 0.  (tests/test_l1_pdch_model.py shows the reference's own
    detector meeting the same condition on the CPU.)"""
    import torch
    sps, fn, F = 4, 9, 30
    A, T = COMB.shape[0], 8 * F
    rng = np.random.default_rng(6)
    m = model(o, lp.UP)
    ins = lp.random_inputs(rng, m, fn, F, p_send=0.75)
    ms, bts = pkg.L1Pdch(ctx, COMB, BSIC, lp.UP), pkg.L1Pdch(ctx, COMB, BSIC, lp.UP)
    out = gpu_encode(ms, fn, F, ins)
    g = ms.collect()
    slots = np.argwhere(g["what"].T != 0)                    # (slot, arfcn) of the bursts on the air
    B = len(slots)
    cell = 160 * sps
    idx = dev((slots[:, 1].astype(np.int64) * T + slots[:, 0]))
    bits = pkg._dev_tensor(ctx, out.d_bits, (A * T, 148), "|u1")[idx].contiguous()
    off = dev(((slots[:, 0] * A + slots[:, 1]) * cell).astype(np.int32))
    x = torch.zeros(T * A * cell, 2, dtype=torch.float32, device="cuda")
    gain = torch.full((B,), 1000.0, dtype=torch.float32, device="cuda")      # above the group's energy gate, which starts at 250
    ctx.modulate(bits, torch.full((B,), 8, dtype=torch.int32, device="cuda"), x, off, gain=gain)
    grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn, 0))
    plan = ms.circuit_plan()
    for a in range(A):
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % (BSIC & 7)] + \
                   ["CMD SETSLOT %d %d" % (tn, 1 if COMB[a, tn] == 13 else plan[a, tn]) for tn in range(8)] + ["CMD POWERON"]:
            grp.control(a, cmd)
    res = grp.pull(x.data_ptr(), A * cell, cell, fn, 0, T)
    grp.sync()
    bts.decode(res, fn)
    r = bts.collect_decode()["pdtch"]
    col = grp.collect()
    assert col["valid"][slots[:, 0], slots[:, 1]].all(), "a clean burst was not detected"
    bf, nb = lp.encode_blocks(lp.PDTCH, fn, F)
    blk0, shown, nclose = lp.decode_blocks(lp.PDTCH, fn, F)
    sent = (ins["kind"] == 1) & (ins["cs"] <= 3)
    checked = 0
    for ci in range(4):
        for b in range(nb):
            j = b + bf - blk0
            if sent[ci, b] and j < nclose:
                assert (r["ok"][ci, j], r["nb"][ci, j], r["cs"][ci, j], r["usf"][ci, j]) == (1, 4, ins["cs"][ci, b], ins["payload"][ci, b, 0] & 7), (ci, b)
                assert np.array_equal(r["payload"][ci, j], ins["payload"][ci, b]), (ci, b)
                checked += 1
            elif not sent[ci, b]:
                assert r["nb"][ci, j] == 0, (ci, b)
    assert checked >= 12 and len(set(ins["cs"][sent])) == 4 and not sent.all()
    same_decode(bts.collect_decode(), model(o, lp.UP).decode(col, fn), "closed loop")
    grp.close(); ms.destroy(); bts.destroy()


# ---- the refusals, last ----
def test_refusals(pkg, ctx, o):
    import ctypes as C
    import torch
    L = pkg.lib()
    h = C.c_void_p()
    comb = np.ascontiguousarray(COMB)
    create = lambda n, cb, bsic, d: L.trxsig_l1pdch_create(C.byref(h), ctx.h, n, cb.ctypes.data if cb is not None else None, bsic, d)
    bad = comb.copy(); bad[1, 2] = 2
    for args in ((3, bad, BSIC, 0), (3, comb, BSIC, 2), (3, comb, BSIC, -1), (0, comb, BSIC, 0), (3, None, BSIC, 0), (3, comb, 64, 0)):
        assert create(*args) == -1 and not h.value, args[0]
    assert b"trxsig_l1pdch_create" in L.trxsig_last_error(ctx.h)
    for v in (3, 4, 6, 12, 14):
        bad = comb.copy(); bad[2, 7] = v
        assert create(3, bad, BSIC, 1) == -1
    obj, up = pkg.L1Pdch(ctx, COMB, BSIC, lp.DOWN), pkg.L1Pdch(ctx, COMB, BSIC, lp.UP)
    assert obj.channels(0) == 4 and L.trxsig_l1pdch_channels(obj.h, 2) == -1 and L.trxsig_l1pdch_channel(obj.h, 0, 4, None, None) == -1
    assert L.trxsig_l1pdch_channel(up.h, 1, 0, None, None) == -1 and L.trxsig_l1pdch_grid(obj.h, HYPER, 4, None, None) == -1
    m = model(o, lp.DOWN)
    ins = lp.random_inputs(np.random.default_rng(1), m, 0, 13)
    t = {k: dev(v) for k, v in ins.items()}
    ok = dict(pdtch_kind=t["kind"], pdtch_cs=t["cs"], pdtch_payload=t["payload"], ptcch_kind=t["pt_kind"], ptcch_payload=t["pt_payload"])
    buf = torch.zeros(3 * 8 * 13 * 149, dtype=torch.uint8, device="cuda")
    for fn, F, kw in ((-1, 13, ok), (HYPER, 13, ok), (0, 0, ok), (0, -4, ok), (0, 13, dict(ok, pdtch_cs=None)), (0, 13, dict(ok, ptcch_payload=None)),
                      (0, 13, dict(ok, bits_onto=buf)), (0, 13, dict(ok, what_onto=buf))):
        with pytest.raises(pkg.TrxSigError, match="trxsig_l1pdch_encode"):
            obj.encode(fn, F, **kw)
    row = torch.full((8 * 4, 3), -1, dtype=torch.int32, device="cuda")
    mk = lambda **kw: pkg.TrxGroupResult(**dict(dict(n_slots=32, n_arfcn=3, n_rows=0, d_row=row.data_ptr(), d_valid=None, d_flags=None,
                                                     d_amp=None, d_toa=None, d_avgpwr=None, d_threshold=None, d_soft=None, soft_stride=148), **kw))
    obj.decode(mk(), 0)                                      # a pull without rows is fine: every block empty
    g = obj.collect_decode()
    assert (g["pdtch"]["nb"] == 0).all() and (g["pdtch"]["cs"] == 255).all() and g["pdtch"]["fn"].shape == (4, 1)
    for res, fn, force in ((mk(n_slots=31), 0, -1), (mk(n_arfcn=2), 0, -1), (mk(), -1, -1), (mk(), HYPER, -1), (mk(), 0, 4), (mk(), 0, -2),
                           (mk(d_row=None), 0, -1), (mk(n_rows=3), 0, -1)):
        with pytest.raises(pkg.TrxSigError, match="trxsig_l1pdch_decode"):
            obj.decode(res, fn, cs_force=force)
    ctx.synchronize()
    obj.destroy(); up.destroy()
