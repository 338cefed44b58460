"""GPU parity of the ciphering stage (trxsig_l1ciph.h) against its model (tests/l1_ciph_model.py): the A5/1 primitive on the
published vector and on random keys; bits() in both directions against the model byte for byte, with and without the encoder's
map, split at frame boundaries, across the hyperframe wrap, past one grid, with a key change between two enqueued calls; soft()
word for word with rows that must not be written; the closed loop at L1 on both legs (every payload back, a wrong key and a
missing decipher fail parity); one loop through samples; the bad-input rules.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _pkg
import fec_stream_model as fsm
import l1_ciph_model as lcm
import l1_ms_model as lms

pytestmark = pytest.mark.gpu
HYPER = lcm.HYPERFRAME
EINVAL = -1
KC = bytes.fromhex("1223456789ABCDEF")
BLOCK1 = bytes.fromhex("534EAA582FE8151AB6E1855A728C00")
BLOCK2 = bytes.fromhex("24FD35A35D5FB6526D32F906DF1AC0")
GOOD = fsm.DECODED | fsm.TCH_GOOD


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


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def small_plan():
    comb = np.zeros((2, 8), np.uint8)
    comb[0, :3] = [5, 7, 1]; comb[1, 0] = 1
    return comb


def keyed(pkg, ctx, rng, comb, every=2):
    """an object and its model with random distinct keys on every `every`-th channel of each class, the rest off"""
    ci, m = pkg.L1Ciph(ctx, comb), lcm.CiphModel(comb)
    keys = set()
    for cls in (lcm.TCH, lcm.XCCH):
        assert ci.channels(cls) == len(m.ch[cls])
        for i in range(0, len(m.ch[cls]), every):
            kc = rng.integers(0, 256, 8).astype(np.uint8)
            assert kc.tobytes() not in keys and kc.any()
            keys.add(kc.tobytes())
            ci.set(cls, i, pkg.A5_1, kc); m.set(cls, i, lcm.A5_1, kc)
    return ci, m


# ---- 1: the primitive ----
def test_primitive(pkg, ctx):
    import torch
    kc, cnt = dev(np.array(list(KC), np.uint8).reshape(1, 8)), dev(np.array([0x134], np.int32))
    b1, b2 = torch.zeros(1, 114, dtype=torch.uint8, device="cuda"), torch.zeros(1, 114, dtype=torch.uint8, device="cuda")
    pkg.a5_1_blocks(ctx, kc, cnt, b1, b2)
    ctx.synchronize()
    assert np.packbits(b1.cpu().numpy()[0]).tobytes() == BLOCK1 and np.packbits(b2.cpu().numpy()[0]).tobytes() == BLOCK2
    rng = np.random.default_rng(11)
    n = 193                                                  # three waves and a lane
    kcs = rng.integers(0, 256, (n, 8)).astype(np.uint8)
    kcs[5] = 0
    counts = rng.integers(0, 1 << 22, n).astype(np.int32)
    counts[5] = 0                                            # the fixed point among them
    w1, w2 = lcm.blocks_batch(kcs, counts)
    SENT = 0xA5
    g = [torch.full((n + 1, 114), SENT, dtype=torch.uint8, device="cuda") for _ in range(4)]
    dk, dc = dev(kcs), dev(counts)
    pkg.a5_1_blocks(ctx, dk, dc, g[0], g[1])
    pkg.a5_1_blocks(ctx, dk, dc, g[2], None)
    pkg.a5_1_blocks(ctx, dk, dc, None, g[3])
    ctx.synchronize()
    h = [x.cpu().numpy() for x in g]
    assert np.array_equal(h[0][:n], w1) and np.array_equal(h[1][:n], w2) and np.array_equal(h[2][:n], w1) and np.array_equal(h[3][:n], w2)
    assert all((x[n] == SENT).all() for x in h) and not w1[5].any() and w1[4].any()
    L = ctx.L
    assert L.trxsig_a5_1_blocks_batch(ctx.h, 0, None, None, None, None) == 0
    for bad in ((-1, dk, dc, g[0], g[1]), (n, None, dc, g[0], g[1]), (n, dk, None, g[0], g[1]), (n, dk, dc, None, None)):
        assert L.trxsig_a5_1_blocks_batch(ctx.h, bad[0], *[None if t is None else t.data_ptr() for t in bad[1:]]) == EINVAL


# ---- 2: bits ----
@pytest.fixture(scope="module")
def bits_case(pkg, ctx):
    """the small plan, half the channels keyed, 104 frames of random bits and a random map, and the model's answers (computed once)"""
    rng = np.random.default_rng(21)
    comb, F, fn = small_plan(), 104, 1326 * 11 - 40
    ci, m = keyed(pkg, ctx, rng, comb)
    bits = rng.integers(0, 2, (2, 8 * F, 148)).astype(np.uint8)
    what = {0: rng.integers(0, 8, (2, 8 * F)).astype(np.uint8), 1: rng.integers(0, 4, (2, 8 * F)).astype(np.uint8)}
    what[0][0, 5] = 200                                      # a code past the mask's width is never eligible
    mask = {0: 1 << pkg.L1TX_XCCH | 1 << pkg.L1TX_TCH, 1: 1 << pkg.L1MS_TCH | 1 << pkg.L1MS_XCCH}
    want = {(up, w): m.bits(up, fn, F, bits, what[up] if w else None, mask[up]) for up in (0, 1) for w in (0, 1)}
    yield dict(ci=ci, m=m, comb=comb, F=F, fn=fn, bits=bits, what=what, mask=mask, want=want)
    ci.destroy()


@pytest.mark.parametrize("uplink", [0, 1])
@pytest.mark.parametrize("with_what", [0, 1])
def test_bits_against_the_model(pkg, ctx, bits_case, uplink, with_what):
    k = bits_case
    ci, F, fn = k["ci"], k["F"], k["fn"]
    want = k["want"][(uplink, with_what)]
    w = dev(k["what"][uplink]) if with_what else None
    mask = k["mask"][uplink]
    d = dev(k["bits"])
    ci.bits(uplink, fn, F, d, w, mask)
    ctx.synchronize()
    got = d.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:8]
    changed = (got != k["bits"]).any(-1)
    on, _ = k["m"].slot_keystream(uplink, fn, F)
    assert changed.sum() > (20 if with_what else 100) and not changed[~on].any()
    if with_what:
        el = (mask >> np.minimum(k["what"][uplink], 31)) & 1
        assert not changed[el == 0].any() and (on & (el == 0)).sum() > 50 and not changed[0, 5]
    rest = np.setdiff1d(np.arange(148), lcm.POS)
    assert len(rest) == 34 and np.array_equal(got[..., rest], k["bits"][..., rest])
    # the same call again deciphers
    ci.bits(uplink, fn, F, d, w, mask)
    # 104 frames in one call = 37 + 67 = 104 single frames (each ARFCN's rows of a part are a slice of the whole's)
    for cuts in ([0, 37, 104], list(range(105))):
        parts = []
        for lo, hi in zip(cuts, cuts[1:]):
            p = dev(k["bits"][:, 8 * lo:8 * hi])
            pw = dev(k["what"][uplink][:, 8 * lo:8 * hi]) if with_what else None
            ci.bits(uplink, (fn + lo) % HYPER, hi - lo, p, pw, mask)
            parts.append((p, pw))
        ctx.synchronize()
        assert np.array_equal(np.concatenate([p.cpu().numpy() for p, _ in parts], axis=1), want), len(cuts)
    assert np.array_equal(d.cpu().numpy(), k["bits"])


@pytest.mark.parametrize("uplink", [0, 1])
def test_bits_across_the_hyperframe_wrap(pkg, ctx, bits_case, uplink):
    k = bits_case
    fn, F = HYPER - 3, 8
    src = k["bits"][:, :8 * F]
    want = k["m"].bits(uplink, fn, F, src)
    d = dev(src)
    k["ci"].bits(uplink, fn, F, d)
    ctx.synchronize()
    got = d.cpu().numpy()
    assert np.array_equal(got, want)
    ch = (got != src).any(-1)
    assert ch[:, :24].any() and ch[:, 24:].any()             # slots of both hyperframes were ciphered


def test_set_takes_effect_in_stream_order(pkg, ctx):
    """bits / set / bits / set(off) / bits enqueued back to back: each call uses the key set before it; the records follow"""
    rng = np.random.default_rng(23)
    comb, F, fn = small_plan(), 26, 4000
    ci, m = pkg.L1Ciph(ctx, comb), lcm.CiphModel(comb)
    assert not ci.collect()["tch"].any() and not ci.collect()["xcch"].any()      # a new object: every channel off
    src = rng.integers(0, 2, (2, 8 * F, 148)).astype(np.uint8)
    k1, k2 = rng.integers(0, 256, 8).astype(np.uint8), rng.integers(0, 256, 8).astype(np.uint8)
    d = [dev(src) for _ in range(4)]
    ci.bits(0, fn, F, d[0])                                  # nothing keyed yet
    ci.set(lcm.TCH, 1, pkg.A5_1, k1); ci.set(lcm.XCCH, 9, pkg.A5_1, k1)
    ci.bits(0, fn, F, d[1])
    ci.set(lcm.TCH, 1, pkg.A5_1, k2)
    ci.bits(0, fn, F, d[2])
    ci.set(lcm.TCH, 1, pkg.A5_OFF); ci.set(lcm.XCCH, 9, pkg.A5_OFF, None)
    ci.bits(0, fn, F, d[3])
    ctx.synchronize()
    got = [x.cpu().numpy() for x in d]
    assert np.array_equal(got[0], src) and np.array_equal(got[3], src)
    m.set(lcm.TCH, 1, lcm.A5_1, k1); m.set(lcm.XCCH, 9, lcm.A5_1, k1)
    w1 = m.bits(0, fn, F, src)
    st = m.state(lcm.TCH).copy()
    m.set(lcm.TCH, 1, lcm.A5_1, k2)
    w2 = m.bits(0, fn, F, src)
    assert np.array_equal(got[1], w1) and np.array_equal(got[2], w2) and not np.array_equal(w1, w2) and not np.array_equal(w1, src)
    ci.set(lcm.TCH, 1, pkg.A5_1, k1)
    r = ci.collect()
    assert np.array_equal(r["tch"], st) and st[1, 0] == 1 and st[1, 1:].all() and not r["xcch"].any()
    ci.destroy()


def test_bits_past_one_grid(pkg, ctx):
    """2 ARFCNs x 32,800 frames = 524,800 slots, past the 2,048 workgroups x 256 lanes of one round of the grid: one call equals
    the same frames in two calls, on the device; the last slots were ciphered."""
    import torch
    comb = np.zeros((2, 8), np.uint8)
    comb[:, 7] = 1
    ci = pkg.L1Ciph(ctx, comb)
    for i in range(2):
        ci.set(lcm.TCH, i, pkg.A5_1, [i + 1] * 8); ci.set(lcm.XCCH, i, pkg.A5_1, [i + 7] * 8)
    F, fn = 32800, HYPER - 20000
    assert 2 * 8 * F > 2048 * 256
    whole = torch.zeros(2, 8 * F, 148, dtype=torch.uint8, device="cuda")
    parts = torch.zeros_like(whole)
    ci.bits(1, fn, F, whole)
    cut = 12345
    lo, hi = parts[:, :8 * cut].contiguous(), parts[:, 8 * cut:].contiguous()
    ci.bits(1, fn, cut, lo)
    ci.bits(1, (fn + cut) % HYPER, F - cut, hi)
    ctx.synchronize()
    assert torch.equal(whole, torch.cat([lo, hi], dim=1))
    per = whole[:, 7::8].any(dim=2).sum(dim=1).cpu().numpy()   # TN 7: every frame but the idle one, one in 26
    assert (per >= F - F // 26 - 2).all() and (per <= F - F // 26 + 1).all() and not whole[:, 0::8].any()
    assert whole[1, 8 * (F - 1) + 7].any() or whole[1, 8 * (F - 2) + 7].any()
    ci.destroy()


# ---- 3: soft ----
def make_result(pkg, row, valid, soft, n_rows=None):
    t = dict(row=dev(row), valid=dev(valid), soft=dev(soft), amp=dev(np.full((len(soft), 2), 1000.0, np.float32)),
             toa=dev(np.zeros(len(soft), np.float32)))
    T, A = row.shape
    res = pkg.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=len(valid) if n_rows is None else n_rows, d_row=t["row"].data_ptr(),
                             d_valid=t["valid"].data_ptr(), d_flags=None, d_amp=t["amp"].data_ptr(), d_toa=t["toa"].data_ptr(),
                             d_avgpwr=None, d_threshold=None, d_soft=t["soft"].data_ptr(), soft_stride=soft.shape[1])
    return res, t


@pytest.mark.parametrize("uplink", [0, 1])
def test_soft_against_the_model(pkg, ctx, bits_case, uplink):
    """Rows in a shuffled order with a stride of 150; values 0.0 / 1.0 with NaN, Inf, negative and large ones among them; slots
    without a row, rows that are not valid, rows at or past n_rows: none of those is written.  Words and NaN positions equal."""
    k = bits_case
    rng = np.random.default_rng(31 + uplink)
    ci, m, F, fn = k["ci"], k["m"], 104, k["fn"] + 3
    T, A = 8 * F, 2
    n = T * A
    row = rng.permutation(n).astype(np.int32).reshape(T, A)
    n_rows = n - 40                                          # the 40 highest row numbers are out of range
    row[rng.random((T, A)) < 0.1] = -1
    valid = (rng.random(n) < 0.85).astype(np.uint8) * pkg.F_DETECT
    soft = rng.integers(0, 2, (n, 150)).astype(np.float32)
    odd = rng.random((n, 150)) < 0.02
    soft[odd] = rng.choice(np.array([np.nan, -np.nan, np.inf, -0.0, -3.5, 0.25, 1e30, 7.0], np.float32), int(odd.sum()))
    want = m.soft(uplink, fn, np.where(row < n_rows, row, -1), valid, soft)
    res, t = make_result(pkg, row, valid, soft, n_rows)
    ci.soft(uplink, res, fn)
    ctx.synchronize()
    got = t["soft"].cpu().numpy()
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), np.argwhere(~same)[:8]
    assert np.array_equal(np.isnan(got), np.isnan(soft))
    touched = (got.view(np.uint32) != soft.view(np.uint32)).any(1)
    assert touched.sum() > 60 and not touched[n_rows:].any() and not touched[valid == 0].any()
    unrowed = np.setdiff1d(np.arange(n), row[row >= 0])
    assert len(unrowed) > 20 and not touched[unrowed].any()
    assert np.array_equal(got[:, 148:].view(np.uint32), soft[:, 148:].view(np.uint32))


# ---- 4: the closed loop at L1 ----
def soft_result(pkg, bits, what):
    """a pull's result made of burst bits: row t * A + a, soft 0.0 / 1.0, valid where something was sent"""
    A, T, _ = bits.shape
    row = np.arange(T * A, dtype=np.int32).reshape(T, A)
    valid = ((what.T != 0).reshape(-1) * 2).astype(np.uint8)
    return make_result(pkg, row, valid, bits.transpose(1, 0, 2).reshape(T * A, 148).astype(np.float32))


def leg(pkg, ctx, uplink, comb, fn, F, grids, keys_tx=None, keys_rx=None, decipher=True):
    """encode -> [bits] -> soft values from bits -> [soft] -> decode on fresh objects; the decoder's outputs.  keys: {(cls, chan): kc}"""
    bsic = 21
    enc = (pkg.L1Ms if uplink else pkg.L1Tx)(ctx, comb, bsic)
    dec = (pkg.L1Rx if uplink else pkg.L1MsRx)(ctx, comb, bsic)
    t = {k: dev(v) for k, v in grids.items()}
    out = enc.encode(fn, F, **t)
    mask = (1 << pkg.L1MS_TCH | 1 << pkg.L1MS_XCCH) if uplink else (1 << pkg.L1TX_XCCH | 1 << pkg.L1TX_TCH)
    objs = []
    if keys_tx is not None:
        ci = pkg.L1Ciph(ctx, comb)
        for (cls, i), kc in keys_tx.items():
            ci.set(cls, i, pkg.A5_1, kc)
        ci.bits(uplink, fn, F, out.d_bits, out.d_what, mask)  # the encoder's own grid, in place
        objs.append(ci)
    r = enc.collect(state=False)
    res, keep = soft_result(pkg, r["bits"], r["what"])
    if keys_rx is not None and decipher:
        ci = pkg.L1Ciph(ctx, comb)
        for (cls, i), kc in keys_rx.items():
            ci.set(cls, i, pkg.A5_1, kc)
        ci.soft(uplink, res, fn)
        objs.append(ci)
    dec.decode(res, fn)
    got = dec.collect(state=False)
    got["_bits"], got["_what"], got["_soft"] = r["bits"], r["what"], keep["soft"].cpu().numpy()
    for o in objs + [enc, dec]:
        o.destroy()
    return got


OUT_KEYS = ("tch_status", "tch", "facch", "tch_fn", "xcch_status", "xcch", "xcch_fn")


@pytest.mark.parametrize("uplink", [0, 1])
def test_closed_loop_at_l1(pkg, ctx, uplink):
    rng = np.random.default_rng(41 + uplink)
    comb, F, fn = small_plan(), 104, 1326 * 5 + 26
    ms_model = lms.MsModel(comb, 21, oracle=object())         # the plan and the walk only
    if uplink:
        grids = lms.grids(ms_model, lms.Content(rng, p_none=0.0, speech=True), fn, F)
        grids["rach_kind"][:] = 1
    else:
        tx = pkg.L1Tx(ctx, comb, 21)
        nbt, nbx, nbc = tx.grid(fn, F)
        nt, nx, nc = tx.channels(pkg.L1_TCH), tx.channels(pkg.L1_XCCH), tx.channels(pkg.L1_CCCH)
        tx.destroy()
        pay = rng.integers(0, 256, (nt, nbt, 33)).astype(np.uint8)
        pay[..., 32] &= 0xF0
        grids = dict(tch_kind=rng.choice(np.array([1, 1, 2], np.uint8), (nt, nbt)), tch_payload=pay,
                     xcch_kind=np.ones((nx, nbx), np.uint8), xcch_payload=rng.integers(0, 256, (nx, nbx, 23)).astype(np.uint8),
                     ccch_kind=np.ones((nc, nbc), np.uint8), ccch_payload=rng.integers(0, 256, (nc, nbc, 23)).astype(np.uint8))
    nt, nx = len(ms_model.ch[lms.TCH]), len(ms_model.ch[lms.XCCH])
    keys = {(lcm.TCH, i): rng.integers(1, 256, 8).astype(np.uint8) for i in range(nt)}
    keys.update({(lcm.XCCH, i): rng.integers(1, 256, 8).astype(np.uint8) for i in range(0, nx, 2)})
    plain = leg(pkg, ctx, uplink, comb, fn, F, grids)
    both = leg(pkg, ctx, uplink, comb, fn, F, grids, keys, keys)
    # the unciphered run decodes: whole XCCH blocks good, TCH blocks good or FACCH
    xg = plain["xcch_status"] == GOOD
    tg = (plain["tch_status"] == GOOD) | ((plain["tch_status"] & fsm.FACCH_OK) != 0)
    fa = (plain["tch_status"] & fsm.FACCH_OK) != 0
    assert xg.sum() > 20 and tg.sum() > 30 and fa.any(axis=1).all()
    # ciphered on the way out ...
    ciphered = (both["_bits"] != plain["_bits"]).any(-1)
    assert ciphered.sum() > 200 and np.array_equal(both["_what"], plain["_what"])
    assert not ciphered[(plain["_what"] != (pkg.L1MS_TCH if uplink else pkg.L1TX_TCH)) &
                        (plain["_what"] != (pkg.L1MS_XCCH if uplink else pkg.L1TX_XCCH))].any()
    # ... the deciphered soft rows are the plain run's, word for word, and so is everything decoded
    assert np.array_equal(both["_soft"].view(np.uint32), plain["_soft"].view(np.uint32))
    for k in OUT_KEYS:
        assert np.array_equal(both[k], plain[k]), k
    # one channel of each class with another key on the receive side: its blocks fail parity, every other channel still decodes
    wrong = dict(keys)
    wx = 2                                                   # an SDCCH of the combination-V slot (keyed: even): two whole blocks
    wrong[(lcm.TCH, 1)] = rng.integers(1, 256, 8).astype(np.uint8)
    wrong[(lcm.XCCH, wx)] = rng.integers(1, 256, 8).astype(np.uint8)
    bad = leg(pkg, ctx, uplink, comb, fn, F, grids, keys, wrong)
    assert xg[wx].sum() >= 2 and not (bad["xcch_status"][wx][xg[wx]] & fsm.TCH_GOOD).any()
    assert not (bad["tch_status"][1][fa[1]] & fsm.FACCH_OK).any()
    others_x = np.arange(nx) != wx
    for k in ("xcch_status", "xcch", "xcch_fn"):
        assert np.array_equal(bad[k][others_x], plain[k][others_x]), k
    for k in ("tch_status", "tch", "facch", "tch_fn"):
        assert np.array_equal(bad[k][0], plain[k][0]), k
    # deciphering left out: every ciphered XCCH block fails parity, the channels that are off decode as before
    raw = leg(pkg, ctx, uplink, comb, fn, F, grids, keys, keys, decipher=False)
    on_x = np.zeros(nx, bool)
    on_x[0::2] = True
    assert xg[on_x].sum() > 8 and not (raw["xcch_status"][on_x][xg[on_x]] & fsm.TCH_GOOD).any()
    for k in ("xcch_status", "xcch", "xcch_fn"):
        assert np.array_equal(raw[k][~on_x], plain[k][~on_x]), k
    assert not (raw["tch_status"][fa] & fsm.FACCH_OK).any()


# ---- 5: through samples ----
def test_uplink_through_samples(pkg):
    """l1ms -> bits(uplink) -> radiate -> noise -> pull -> soft(uplink) -> l1rx on the small plan, with the helpers of
    tests/test_gpu_l1ms.py's closed loop: the same blocks decode to the same payloads as in the unciphered run."""
    import test_gpu_l1ms as tms
    sps, A, F, fn0, bsic, band = 4, 2, 104, 26 * 40, 21, 1800
    comb = small_plan()
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    model = lms.MsModel(comb, bsic, band, oracle=object())
    rng = np.random.default_rng(51)
    g = lms.grids(model, lms.Content(rng, p_none=0.1, speech=True), fn0, F)
    half = lambda n: rng.uniform(-0.5, 0.5, n) / sps
    air = tms.Air(rng, model, len(g["rach_kind"]), half, half)
    nt, nx = len(model.ch[lms.TCH]), len(model.ch[lms.XCCH])
    keys = {(lcm.TCH, i): rng.integers(1, 256, 8).astype(np.uint8) for i in range(nt)}
    keys.update({(lcm.XCCH, i): rng.integers(1, 256, 8).astype(np.uint8) for i in range(0, nx, 2)})
    mask = 1 << pkg.L1MS_TCH | 1 << pkg.L1MS_XCCH
    runs = []
    for cipher in (False, True):
        ms, rx, ci = pkg.L1Ms(ctx, comb, bsic, band), pkg.L1Rx(ctx, comb, bsic, band), pkg.L1Ciph(ctx, comb)
        for (cls, i), kc in keys.items():
            ci.set(cls, i, pkg.A5_1, kc)
        t = {k: tms.dev(v) for k, v in g.items()}
        out = ms.encode(fn0, F, **t)
        if cipher:
            ci.bits(1, fn0, F, out.d_bits, out.d_what, mask)
        r = ms.collect(state=False)
        buf, cell = tms.radiate_with_noise(ms, air, r["what"], A, F, sps, seed=52)
        grp = tms.setup_group(pkg, ctx, comb, bsic & 7, fn0)
        res = grp.pull(buf.data_ptr(), A * cell, cell, fn0, 0, 8 * F)
        grp.sync()
        if cipher:
            ci.soft(1, res, fn0)
        rx.decode(res, fn0)
        got = rx.collect(state=False)
        col = grp.collect()
        sent = np.argwhere(r["what"].T != 0)
        assert all(col["valid"][s, a] for s, a in sent), "a clean burst was not detected"
        got["_bits"] = r["bits"]
        runs.append(got)
        ms.destroy(); rx.destroy(); ci.destroy(); grp.close()
    plain, ciph = runs
    assert ((plain["_bits"] != ciph["_bits"]).any(-1)).sum() > 150
    xg = plain["xcch_status"] == GOOD
    tg = (plain["tch_status"] == GOOD) | ((plain["tch_status"] & fsm.FACCH_OK) != 0)
    assert xg.sum() > 15 and tg.sum() > 30
    for k in ("tch_status", "tch_fn", "xcch_status", "xcch_fn", "xcch"):
        assert np.array_equal(plain[k], ciph[k]), k
    assert np.array_equal(plain["tch"][tg], ciph["tch"][tg]) and np.array_equal(plain["facch"][tg], ciph["facch"][tg])
    assert np.array_equal(plain["rach"]["ra"], ciph["rach"]["ra"]) and len(plain["rach"]["ra"]) > 10
    ctx.close()


# ---- 6: the bad-input rules ----
def test_bad_inputs(pkg, ctx):
    """Each returns TRXSIG_EINVAL with nothing launched."""
    import torch
    L = ctx.L
    comb = small_plan()
    for bad in (np.array([[4, 0, 0, 0, 0, 0, 0, 0]], np.uint8), np.array([[0, 5, 0, 0, 0, 0, 0, 0]], np.uint8),
                np.array([[0] * 8, [5] + [0] * 7], np.uint8)):
        with pytest.raises(pkg.TrxSigError):
            pkg.L1Ciph(ctx, bad)
    h = C.c_void_p()
    assert L.trxsig_l1ciph_create(C.byref(h), ctx.h, 0, comb.ctypes.data) == EINVAL
    assert L.trxsig_l1ciph_create(C.byref(h), ctx.h, 2, None) == EINVAL and not h.value
    ci = pkg.L1Ciph(ctx, comb)
    assert [ci.channels(c) for c in (0, 1)] == [2, 26] and L.trxsig_l1ciph_channels(ci.h, 2) == EINVAL
    rx = pkg.L1Rx(ctx, comb, 1)
    assert all(ci.channel(c, i) == rx.channel(c, i) for c in (0, 1) for i in range(ci.channels(c)))
    rx.destroy()
    assert L.trxsig_l1ciph_channel(ci.h, 0, 2, None, None, None, None) == EINVAL
    assert L.trxsig_l1ciph_channel(ci.h, 2, 0, None, None, None, None) == EINVAL
    key = (C.c_uint8 * 8)(*range(1, 9))
    for cls, chan, algo, kc in ((2, 0, 1, key), (0, 2, 1, key), (1, -1, 1, key), (1, 26, 0, None), (0, 0, 2, key), (0, 0, -1, key),
                                (0, 0, 1, None)):
        assert L.trxsig_l1ciph_set(ci.h, cls, chan, algo, kc) == EINVAL, (cls, chan, algo)
    assert L.trxsig_l1ciph_set(ci.h, 0, 0, 0, None) == 0 and L.trxsig_l1ciph_set(ci.h, 1, 25, 1, key) == 0
    p = C.c_void_p()
    assert L.trxsig_l1ciph_state(ci.h, 2, C.byref(p)) == EINVAL and L.trxsig_l1ciph_state(ci.h, 0, None) == EINVAL
    ci.set(0, 1, pkg.A5_1, list(range(8)))
    src = np.ones((2, 16, 148), np.uint8)
    d = dev(src)
    a = d.data_ptr()
    for up, fn, F, ptr in ((0, -1, 2, a), (0, HYPER, 2, a), (0, 0, 0, a), (0, 0, -3, a), (0, 0, 1 << 27, a), (2, 0, 2, a), (-1, 0, 2, a),
                           (0, 0, 2, None), (0, 0, 2, a + 2)):
        assert L.trxsig_l1ciph_bits(ci.h, up, fn, F, ptr, None, 0) == EINVAL, (up, fn, F)
    row = np.arange(32, dtype=np.int32).reshape(16, 2)
    res, t = make_result(pkg, row, np.full(32, 2, np.uint8), np.ones((32, 148), np.float32))
    for field, v in (("n_slots", 12), ("n_slots", 0), ("n_arfcn", 1), ("soft_stride", 100), ("d_row", None), ("n_rows", -1),
                     ("d_soft", None), ("d_valid", None)):
        r = pkg.TrxGroupResult(); C.pointer(r)[0] = res
        setattr(r, field, v)
        assert L.trxsig_l1ciph_soft(ci.h, 0, C.byref(r), 0) == EINVAL, field
    assert L.trxsig_l1ciph_soft(ci.h, 0, C.byref(res), HYPER) == EINVAL and L.trxsig_l1ciph_soft(ci.h, 0, C.byref(res), -1) == EINVAL
    assert L.trxsig_l1ciph_soft(ci.h, 2, C.byref(res), 0) == EINVAL and L.trxsig_l1ciph_soft(ci.h, 0, None, 0) == EINVAL
    ctx.synchronize()
    assert np.array_equal(d.cpu().numpy(), src) and (t["soft"].cpu().numpy() == 1.0).all()      # nothing was launched
    r = pkg.TrxGroupResult(); C.pointer(r)[0] = res
    r.n_rows = 0                                             # a pull that returned nothing: OK, nothing to do
    assert L.trxsig_l1ciph_soft(ci.h, 0, C.byref(r), 0) == 0
    ci.bits(0, 0, 2, d)                                      # and good calls still go through
    ci.soft(0, res, 0)
    ctx.synchronize()
    assert (d.cpu().numpy() != src).any() and (t["soft"].cpu().numpy() != 1.0).any()
    ci.destroy()


# ---- 7: one numbering for every stage ----
def test_one_numbering_across_the_stages(pkg):
    """The five stages that number a plan's channels take the numbering from one place (csrc/trxsig_plan.h): on one plan, the
    TCH and XCCH classes are the same channels in the same order in all five, the CCCH in both downlink stages and the RACH in
    both uplink stages.  And the objects' common end (trx_object_destroy): a context destroyed while an object still lives on it
    goes when that object goes, not before."""
    comb = np.array([[5, 7, 1, 0, 1, 7, 0, 1], [7, 1, 1, 0, 0, 1, 7, 0]], np.uint8)
    ctx = pkg.TrxSig(4, 0)
    rx, tx, ms = pkg.L1Rx(ctx, comb, 1), pkg.L1Tx(ctx, comb, 1), pkg.L1Ms(ctx, comb, 1)
    mr, ci = pkg.L1MsRx(ctx, comb, 1), pkg.L1Ciph(ctx, comb)
    objs = (rx, tx, ms, mr, ci)
    ones, fives, sevens = [int((comb == k).sum()) for k in (1, 5, 7)]
    for cls, n in ((pkg.L1_TCH, ones), (pkg.L1_XCCH, 8 * fives + 16 * sevens + ones)):
        assert [o.channels(cls) for o in objs] == [n] * 5
        for i in range(n):
            want = rx.channel(cls, i)
            assert [o.channel(cls, i) for o in objs] == [want] * 5, (cls, i)
    assert tx.channels(pkg.L1_CCCH) == mr.channels(pkg.L1_CCCH) == 3
    assert [tx.channel(pkg.L1_CCCH, i) for i in range(3)] == [mr.channel(pkg.L1_CCCH, i) for i in range(3)] == \
        [(0, 0, pkg.L1_CCCH_C5, i) for i in range(3)]
    assert rx.channels(pkg.L1_RACH) == ms.channels(pkg.L1_RACH) == 1
    assert rx.channel(pkg.L1_RACH, 0) == ms.channel(pkg.L1_RACH, 0) == (0, 0, pkg.L1_RACH_C5, 0)
    # a second context, destroyed under a live object: the object's next call (a launch on that context's stream) succeeds
    import torch
    ctx2 = pkg.TrxSig(4, 0)
    held = pkg.L1Ciph(ctx2, comb)
    ctx2.close()
    key = (C.c_uint8 * 8)(*range(1, 9))
    assert ctx.L.trxsig_l1ciph_set(held.h, pkg.L1_XCCH, 5, pkg.A5_1, key) == 0
    torch.cuda.synchronize()
    assert held.channel(pkg.L1_XCCH, 5) == ci.channel(pkg.L1_XCCH, 5)
    held.destroy()                                           # the context goes with it
    for o in objs:                                           # creation order, the context last
        o.destroy()
    ctx.close()
