"""GPU parity of the uplink stream decoders (trxsig_fec_tch_decode_stream / trxsig_fec_xcch_decode_stream, k_fec_rx_stream +
k_fec_rx_fold) through the C-ABI against the literal CPU model (tests/fec_stream_model.py): status, frames, FER and the state
bytes, exactly.  Random multi-channel streams with missing bursts (closing bursts, whole blocks, gaps across calls, a fresh
decoder's first block), stolen blocks, both wire settings, both B phases, chaining at every block boundary, open(), the
batch decoders where every burst is present, the bad-input rules, unaligned outputs, a closed loop on the card and a
Transceiver group pull."""

import numpy as np
import pytest

import _pkg
import fec_stream_model as fsm
import fectxbind
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def t(pkg):
    c = pkg.TrxSig(4, 0)
    c.use_torch_stream()
    return c


@pytest.fixture(scope="module")
def prims():
    return fsm.Prims()


@pytest.fixture(scope="module")
def tx():
    return fectxbind.FecTxOracle()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def state_bytes(tch):
    return fsm.TCH_STATE_BYTES if tch else fsm.XCCH_STATE_BYTES


def gpu_stream(t, tch, rows, index, state, b0=None, wire=True, fer=True):
    """One stream-decoder call on device copies; every output poisoned first.  Returns host arrays in the model's layout."""
    import torch
    S, T = index.shape
    nb = T // 4
    st = dev(np.asarray(state, np.uint8))
    status = torch.full((S, nb), 0xEE, dtype=torch.uint8, device="cuda")
    tch33 = torch.full((S, nb, 33), 0xEE, dtype=torch.uint8, device="cuda")
    l2 = torch.full((S, nb, 23), 0xEE, dtype=torch.uint8, device="cuda")
    f = torch.full((S, nb), float("nan"), dtype=torch.float32, device="cuda") if fer else None
    soft = rows if isinstance(rows, torch.Tensor) else dev(np.asarray(rows, np.float32))
    idx = dev(np.asarray(index, np.int32))
    if tch:
        t.fec_tch_decode_stream(soft, idx, st, status, tch33, l2, b0=None if b0 is None else dev(np.asarray(b0, np.uint8)), fer=f,
                                wire=wire)
    else:
        t.fec_xcch_decode_stream(soft, idx, st, status, l2, fer=f, wire=wire)
    torch.cuda.synchronize()
    out = dict(status=status.cpu().numpy(), l2=l2.cpu().numpy(), state=st.cpu().numpy())
    if tch:
        out["tch"] = tch33.cpu().numpy()
    if fer:
        out["fer"] = f.cpu().numpy()
    return out


def same(g, m, what=""):
    for k in ("status", "tch", "l2", "fer", "state"):
        if k not in g:
            continue
        a, b = g[k], m[k]
        if k == "fer":
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5])


def stream_case(rng, tx, fo, tch, S, n, p_miss):
    """Bursts, a shuffled row order and an index with the missing patterns the contract names."""
    if tch:
        soft, _, _ = fsm.tch_bursts(rng, tx, S, n, noise=0.35, p_junk=0.05)
    else:
        soft, _ = fsm.xcch_bursts(rng, fo, S, n, noise=0.35)
    T = 4 * n
    rows = soft.reshape(S * T, 148)
    perm = rng.permutation(S * T)
    rows = rows[perm]
    inv = np.empty_like(perm); inv[perm] = np.arange(S * T)
    index = inv.reshape(S, T).astype(np.int64)
    index[rng.random((S, T)) < p_miss] = -1
    index[0, 3::4] = -1                                       # every closing burst of channel 0 missing
    index[1, 4:12] = -1                                       # two whole blocks missing
    index[2, 0:4] = -1                                        # a fresh decoder's first block missing
    index[3, :] = -1                                          # a silent channel
    index[4, T - 6:] = -1                                     # a gap across the end of the call
    index[5, 1] = S * T                                       # indices outside [-1, n_rows): no burst
    index[5, 2] = -7
    index[5, 5] = 2 ** 31 - 1
    return rows, index.astype(np.int32)


@pytest.mark.parametrize("tch", [True, False])
@pytest.mark.parametrize("wire", [True, False])
def test_random_streams_vs_model(t, tx, prims, tch, wire):
    rng = np.random.default_rng(100 + 2 * tch + wire)
    S, n = 24, 6
    rows, index = stream_case(rng, tx, prims.fo, tch, S, n, 0.15)
    b0 = rng.choice([0, 4], S).astype(np.uint8) if tch else None
    st = np.zeros((S, state_bytes(tch)), np.uint8)
    # two calls: the second starts from the state the first left (gaps spanning the boundary included)
    for call in range(2):
        g = gpu_stream(t, tch, rows, index, st, b0=b0, wire=wire)
        m = fsm.run(prims, tch, rows, index, st, b0=b0, wire=wire)
        same(g, m, ("call", call))
        st = g["state"]
        index = np.roll(index, 3, axis=0)
        index[4, :5] = -1                                     # channel 4's gap goes on into the next call
    flags = m["status"]
    assert (flags & fsm.DECODED).any() and (flags & fsm.TCH_GOOD).any() and not (flags & fsm.DECODED).all()
    if tch:
        assert (flags & fsm.STOLEN).any() and (flags & fsm.FACCH_OK).any()


@pytest.mark.parametrize("tch", [True, False])
def test_chaining_at_every_block_boundary(t, tx, prims, tch):
    rng = np.random.default_rng(7 + tch)
    S, n = 8, 8
    rows, index = stream_case(rng, tx, prims.fo, tch, S, n, 0.2)
    b0 = rng.choice([0, 4], S).astype(np.uint8) if tch else None
    st0 = np.zeros((S, state_bytes(tch)), np.uint8)
    whole = gpu_stream(t, tch, rows, index, st0, b0=b0)
    same(whole, fsm.run(prims, tch, rows, index, st0, b0=b0), "whole")
    for k in range(1, n):
        a = gpu_stream(t, tch, rows, index[:, :4 * k], st0, b0=b0)
        b = gpu_stream(t, tch, rows, index[:, 4 * k:], a["state"], b0=None if b0 is None else (b0 + 4 * k) % 8)
        for key in ("status", "tch", "l2", "fer"):
            if key in whole:
                assert np.array_equal(np.concatenate([a[key], b[key]], axis=1), whole[key]), (k, key)
        assert np.array_equal(b["state"], whole["state"]), k


def test_open_resets_fer_and_keeps_rows(t, tx, prims):
    rng = np.random.default_rng(17)
    S, n = 6, 4
    rows, index = stream_case(rng, tx, prims.fo, True, S, n, 0.1)
    first = gpu_stream(t, True, rows, index, np.zeros((S, fsm.TCH_STATE_BYTES), np.uint8))
    assert (first["state"][:, :4].view(np.float32) > 0).any()
    st = first["state"].copy()
    st[:, :4] = 0                                             # L1Decoder::open(): mFER = 0, mI kept
    silent = np.full((S, 4), -1, np.int32)
    g = gpu_stream(t, True, rows, silent, st)
    assert np.array_equal(g["state"], st) and not g["status"].any() and (g["fer"] == 0).all()
    g = gpu_stream(t, True, rows, index, st)
    same(g, fsm.run(prims, True, rows, index, st), "after open")


def test_all_present_agrees_with_the_batch_decoders(t, tx, prims):
    import torch
    rng = np.random.default_rng(23)
    S, n = 4, 12
    soft, _, _ = fsm.tch_bursts(rng, tx, S, n, noise=0.4, p_junk=0.1)
    rows = soft.reshape(S * 4 * n, 148)
    index = np.arange(S * 4 * n, dtype=np.int32).reshape(S, 4 * n)
    g = gpu_stream(t, True, rows, index, np.zeros((S, fsm.TCH_STATE_BYTES), np.uint8), b0=np.zeros(S, np.uint8))
    for s in range(S):
        nb = n - 1
        tch = torch.zeros(nb, 33, dtype=torch.uint8, device="cuda"); good = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        stolen = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        facch = torch.zeros(nb, 23, dtype=torch.uint8, device="cuda"); fok = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        t.fec_tch_decode(dev(soft[s]), 4 * n, tch, good, stolen, facch=facch, facch_ok=fok, wire=True)
        torch.cuda.synchronize()
        st = g["status"][s, 1:]
        sto = stolen.cpu().numpy() != 0
        assert np.array_equal((st & fsm.STOLEN) != 0, sto)
        assert np.array_equal(g["tch"][s, 1:][~sto], tch.cpu().numpy()[~sto])
        assert np.array_equal((st[~sto] & fsm.TCH_GOOD) != 0, good.cpu().numpy()[~sto] != 0)
        assert np.array_equal(g["l2"][s, 1:][sto], facch.cpu().numpy()[sto])
        assert np.array_equal((st[sto] & fsm.FACCH_OK) != 0, fok.cpu().numpy()[sto] != 0)
    xs, _ = fsm.xcch_bursts(rng, prims.fo, S, n, noise=0.45)
    rows = xs.reshape(S * 4 * n, 148)
    g = gpu_stream(t, False, rows, index, np.zeros((S, fsm.XCCH_STATE_BYTES), np.uint8))
    frames = torch.zeros(S * n, 23, dtype=torch.uint8, device="cuda"); ok = torch.zeros(S * n, dtype=torch.uint8, device="cuda")
    t.fec_xcch_decode(dev(rows), S * n, frames, ok, wire=True)
    torch.cuda.synchronize()
    assert np.array_equal(g["l2"].reshape(S * n, 23), frames.cpu().numpy())
    assert np.array_equal(g["status"].ravel(), fsm.DECODED | np.where(ok.cpu().numpy() != 0, fsm.TCH_GOOD, 0))


def test_bad_inputs(pkg, t, tx, prims):
    import torch
    L, h = t.L, t.h
    EINVAL = -1
    rows = dev(np.full((8, 148), 0.25, np.float32))
    idx = dev(np.zeros((2, 8), np.int32))
    st = torch.zeros(2, fsm.TCH_STATE_BYTES, dtype=torch.uint8, device="cuda")
    stat = torch.zeros(2, 2, dtype=torch.uint8, device="cuda")
    o33 = torch.zeros(2, 2, 33, dtype=torch.uint8, device="cuda"); o23 = torch.zeros(2, 2, 23, dtype=torch.uint8, device="cuda")
    P = lambda x: None if x is None else x.data_ptr()

    def tch(n_chan=2, n_slots=8, soft=rows, stride=148, n_rows=8, index=idx, state=st, status=stat, a=o33, b=o23, state_off=0):
        return L.trxsig_fec_tch_decode_stream(h, n_chan, n_slots, P(soft), stride, n_rows, P(index), None, 1,
                                              None if state is None else state.data_ptr() + state_off, P(status), P(a), P(b), None)

    def xcch(n_chan=2, n_slots=8, soft=rows, stride=148, n_rows=8, index=idx, state=st, status=stat, b=o23):
        return L.trxsig_fec_xcch_decode_stream(h, n_chan, n_slots, P(soft), stride, n_rows, P(index), 1, P(state), P(status),
                                               P(b), None)
    assert tch() == 0 and xcch() == 0
    for kw in (dict(soft=None), dict(index=None), dict(state=None), dict(status=None), dict(a=None), dict(b=None),
               dict(n_chan=-1), dict(n_slots=-4), dict(n_rows=-1), dict(n_slots=6), dict(stride=147), dict(n_chan=2 ** 29, n_slots=4),
               dict(state_off=2)):
        assert tch(**kw) == EINVAL, kw
        if "a" not in kw and "state_off" not in kw:
            assert xcch(**kw) == EINVAL, kw
    st_before = st.clone()
    stat.fill_(0xEE)
    assert tch(n_chan=0) == 0 and tch(n_slots=0) == 0 and xcch(n_chan=0, soft=None, index=None) == 0
    torch.cuda.synchronize()
    assert (stat == 0xEE).all() and torch.equal(st, st_before)
    # d_b0 other than 0 / 4: the channel is one where no burst arrives; out-of-range indices: no burst (both on the device)
    rng = np.random.default_rng(29)
    S, n = 6, 4
    r, index = stream_case(rng, tx, prims.fo, True, S, n, 0.0)
    b0 = np.array([0, 1, 4, 7, 200, 3], np.uint8)
    st0 = np.zeros((S, fsm.TCH_STATE_BYTES), np.uint8)
    st0[:, 16:] = rng.random((S, 8 * 114)).astype(np.float32).view(np.uint8).reshape(S, -1)
    st0[:, :4] = np.float32(0.25).reshape(1).view(np.uint8)
    g = gpu_stream(t, True, r, index, st0, b0=b0)
    same(g, fsm.run(prims, True, r, index, st0, b0=b0), "bad b0")
    bad = np.isin(b0, (0, 4), invert=True)
    assert not g["status"][bad].any() and np.array_equal(g["state"][bad], st0[bad])


def test_unaligned_outputs(t, tx, prims):
    import torch
    rng = np.random.default_rng(31)
    S, n = 7, 4
    rows, index = stream_case(rng, tx, prims.fo, True, S, n, 0.1)
    st0 = np.zeros((S, fsm.TCH_STATE_BYTES), np.uint8)
    m = fsm.run(prims, True, rows, index, st0)
    nb = n
    buf = torch.full((S * nb * (1 + 33 + 23 + 4) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    p_stat, p_tch = base + 1, base + 3 + S * nb
    p_l2 = p_tch + S * nb * 33 + 5
    p_fer = p_l2 + S * nb * 23 + 3
    st, d_rows, d_index = dev(st0), dev(rows), dev(index)    # held: the call is asynchronous
    r = t.L.trxsig_fec_tch_decode_stream(t.h, S, 4 * n, d_rows.data_ptr(), 148, rows.shape[0], d_index.data_ptr(), None, 1,
                                         st.data_ptr(), p_stat, p_tch, p_l2, p_fer)
    assert r == 0
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    o = lambda p, k: h[p - base:p - base + k]
    assert np.array_equal(o(p_stat, S * nb), m["status"].ravel())
    assert np.array_equal(o(p_tch, S * nb * 33), m["tch"].ravel())
    assert np.array_equal(o(p_l2, S * nb * 23), m["l2"].ravel())
    assert np.array_equal(o(p_fer, S * nb * 4), m["fer"].ravel().view(np.uint8))
    assert np.array_equal(st.cpu().numpy(), m["state"])
    assert h[0] == 0xEE and h[p_tch - base - 1] == 0xEE and h[p_l2 - base - 1] == 0xEE


def test_closed_loop_on_the_card(pkg, t, prims):
    """trxsig_fec_tch_encode_batch streams (speech and FACCH) -> GMSK modulate -> noise -> detect + demodulate -> the stream
    decoder: with b0 = 0, stream block m+1 carries encoded block m; every payload and FACCH frame comes back, and the result
    equals the model on the same soft bits."""
    import torch
    sps, tsc, S, n = 4, 3, 4, 24
    rng = np.random.default_rng(37)
    kind = np.where(rng.random((S, n)) < 0.25, pkg.TCH_FACCH, pkg.TCH_SPEECH).astype(np.uint8)
    pl = rng.integers(0, 256, (S, n, 33)).astype(np.uint8)
    pl[:, :, 32] &= 0xF0
    bits = torch.zeros(S, n, 4, 148, dtype=torch.uint8, device="cuda")
    est = torch.zeros(S, 32, dtype=torch.uint8, device="cuda")
    t.fec_tch_encode(dev(kind), dev(pl), dev(np.full(S, tsc, np.uint8)), est, bits)
    B = S * 4 * n
    bits = bits.view(B, 148)
    g = torch.Generator(device="cuda"); g.manual_seed(38)
    guard = torch.full((B,), 8, dtype=torch.int32, device="cuda")
    ns = sps * 156
    off = (torch.arange(B, dtype=torch.int32, device="cuda") * ns).contiguous()
    length = torch.full((B,), ns, dtype=torch.int32, device="cuda")
    x = torch.zeros(B * ns, 2, dtype=torch.float32, device="cuda")
    t.modulate(bits, guard, x, off)
    x += 0.15 * torch.randn(x.shape, device="cuda", generator=g)
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = torch.zeros(B, 2, device="cuda"); toa = torch.zeros(B, device="cuda")
    soft = torch.zeros(B, 148, device="cuda")
    t.detect_demod_normal(x, off, length, tsc, flags, amp, toa, soft, nsoft=148, soft_stride=148)
    torch.cuda.synchronize()
    assert bool(((flags & pkg.F_DETECT) != 0).all())
    index = np.arange(B, dtype=np.int32).reshape(S, 4 * n)
    st0 = np.zeros((S, fsm.TCH_STATE_BYTES), np.uint8)
    out = gpu_stream(t, True, soft, index, st0, b0=np.zeros(S, np.uint8))
    same(out, fsm.run(prims, True, soft.cpu().numpy(), index, st0, b0=np.zeros(S, np.uint8)), "closed loop")
    st = out["status"][:, 1:]
    k = kind[:, :n - 1]
    sp, fa = k == pkg.TCH_SPEECH, k == pkg.TCH_FACCH
    assert (st & fsm.DECODED).all()
    assert np.array_equal((st & fsm.STOLEN) != 0, fa)
    assert ((st[sp] & fsm.TCH_GOOD) != 0).all() and np.array_equal(out["tch"][:, 1:][sp], pl[:, :n - 1][sp])
    assert ((st[fa] & fsm.FACCH_OK) != 0).all() and np.array_equal(out["l2"][:, 1:][fa], pl[:, :n - 1, :23][fa])


def test_fed_from_a_transceiver_group_pull(pkg, t, prims):
    """Traffic bursts on every timeslot of two ARFCNs, some replaced by noise, through trxsig_trxgroup_pull; the index is
    built on the device from the result's d_row / d_valid (-1 where the pull returned nothing) and points into res.d_soft.
    The decode equals the model fed with what trxsig_trxgroup_collect returns."""
    import torch
    from openbts_ttsou_amd.frontend import _DevView
    sps, tsc, A, n = 4, 3, 2, 6
    C8 = 8 * A                                                # channels: (ARFCN a, timeslot tn) -> c = 8a + tn
    rng = np.random.default_rng(41)
    kind = np.where(rng.random((C8, n)) < 0.25, pkg.TCH_FACCH, pkg.TCH_SPEECH).astype(np.uint8)
    pl = rng.integers(0, 256, (C8, n, 33)).astype(np.uint8)
    pl[:, :, 32] &= 0xF0
    bits = torch.zeros(C8, n, 4, 148, dtype=torch.uint8, device="cuda")
    t.fec_tch_encode(dev(kind), dev(pl), dev(np.full(C8, tsc, np.uint8)), torch.zeros(C8, 32, dtype=torch.uint8, device="cuda"), bits)
    hb = bits.cpu().numpy().reshape(C8, 4 * n, 148)
    T = 8 * 4 * n                                             # timeslots
    cell = 160 * sps
    x = np.zeros((T, A, cell), np.complex64)
    drop = rng.random((T, A)) < 0.12
    bb = np.zeros((T * A, 148), np.uint8)
    for slot in range(T):
        for a in range(A):
            bb[slot * A + a] = hb[8 * a + slot % 8, slot // 8]
    xs, offs, lens, _ = synth.bursts_from_bits(bb, sps, seed=42, sigmas=(0.0, 0.05), max_delay=0.5)
    for slot in range(T):
        for a in range(A):
            i = slot * A + a
            nsmp = (156 + (slot % 8 % 4 == 0)) * sps
            if drop[slot, a]:
                x[slot, a, :nsmp] = (rng.standard_normal(nsmp) + 1j * rng.standard_normal(nsmp)) * 0.5
            else:
                v = xs[offs[i]:offs[i] + lens[i]][:nsmp]
                x[slot, a, :len(v)] = v
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD, start=(0, 0))
    for a in range(A):
        for c in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % tsc] + ["CMD SETSLOT %d 1" % tn for tn in range(8)] + \
                 ["CMD POWERON"]:
            grp.control(a, c)
    dx = torch.from_numpy(x.view(np.float32).reshape(-1)).to("cuda:0")
    res = grp.pull(dx.data_ptr(), A * cell, cell, 0, 0, T)
    grp.sync()                                                # d_valid complete on the context's stream
    row = torch.as_tensor(_DevView(res.d_row, (T, A), "<i4"), device="cuda")
    valid = torch.as_tensor(_DevView(res.d_valid, (max(res.n_rows, 1),), "|u1"), device="cuda")
    ok = (row >= 0) & (valid[row.clamp(min=0).long()] != 0)
    idx_ta = torch.where(ok, row, torch.full_like(row, -1))   # [T][A]
    index = idx_ta.view(4 * n, 8, A).permute(2, 1, 0).reshape(C8, 4 * n).contiguous()   # channel 8a + tn, slot k = T/8 index
    st = torch.zeros(C8, fsm.TCH_STATE_BYTES, dtype=torch.uint8, device="cuda")
    nb = n
    status = torch.full((C8, nb), 0xEE, dtype=torch.uint8, device="cuda")
    o33 = torch.full((C8, nb, 33), 0xEE, dtype=torch.uint8, device="cuda"); o23 = torch.full((C8, nb, 23), 0xEE, dtype=torch.uint8, device="cuda")
    fer = torch.zeros(C8, nb, dtype=torch.float32, device="cuda")
    ctx.fec_tch_decode_stream(res.d_soft, index, st, status, o33, o23, fer=fer, n_rows=res.n_rows, soft_stride=res.soft_stride)
    torch.cuda.synchronize()
    col = grp.collect()
    rows = col["soft"].reshape(T * A, 148)
    mi = np.full((C8, 4 * n), -1, np.int32)
    for c in range(C8):
        a, tn = divmod(c, 8)
        for k in range(4 * n):
            if col["valid"][8 * k + tn, a]:
                mi[c, k] = (8 * k + tn) * A + a
    assert (mi >= 0).mean() > 0.7 and (mi < 0).any()
    assert np.array_equal(index.cpu().numpy() >= 0, mi >= 0)
    m = fsm.run(prims, True, rows, mi, np.zeros((C8, fsm.TCH_STATE_BYTES), np.uint8))
    g = dict(status=status.cpu().numpy(), tch=o33.cpu().numpy(), l2=o23.cpu().numpy(), fer=fer.cpu().numpy(), state=st.cpu().numpy())
    same(g, m, "group pull")
    assert (g["status"] & fsm.TCH_GOOD).any()
    grp.close(); ctx.close()


# ---- production scale: the shapes tools/fec_stream_bench.py times, the ragged last workgroup, long gaps, index edges ----
def long_stream(rng, tx, fo, tch, S, n_total):
    """S channels x n_total blocks of bursts as one row buffer (rows in shuffled order) and the full index [S, 4 n_total]."""
    if tch:
        soft, _, _ = fsm.tch_bursts(rng, tx, S, n_total, noise=0.35, p_junk=0.05)
    else:
        soft, _ = fsm.xcch_bursts(rng, fo, S, n_total, noise=0.35)
    T = 4 * n_total
    perm = rng.permutation(S * T)
    rows = soft.reshape(S * T, 148)[perm]
    inv = np.empty_like(perm); inv[perm] = np.arange(S * T)
    return rows, inv.reshape(S, T).astype(np.int64)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tch", [True, False])
@pytest.mark.parametrize("wire", [True, False])
def test_production_shape_vs_model(t, tx, prims, tch, wire):
    """1,024 channels x 16 blocks in one call (the bench's shape), from a state with random rows and FER, with the missing
    patterns of stream_case and random drops."""
    rng = np.random.default_rng(400 + 2 * tch + wire)
    S, n = 1024, 16
    rows, index = stream_case(rng, tx, prims.fo, tch, S, n, 0.1)
    b0 = rng.choice([0, 4], S).astype(np.uint8) if tch else None
    st = np.zeros((S, state_bytes(tch)), np.uint8)
    st[:, fsm.HDR:] = rng.random((S, (state_bytes(tch) - fsm.HDR) // 4)).astype(np.float32).view(np.uint8)
    st[:, :4] = rng.random(S).astype(np.float32).reshape(S, 1).view(np.uint8)
    g = gpu_stream(t, tch, rows, index, st, b0=b0, wire=wire)
    m = fsm.run(prims, tch, rows, index, st, b0=b0, wire=wire)
    same(g, m, "production shape")
    assert S * n == 16384 and (m["status"] & fsm.TCH_GOOD).mean() > 0.5 and not (m["status"] & fsm.DECODED).all()


def gap_plan(rng, S, T, calls, P):
    """Missing-burst gaps of 3..10 periods for most channels: across block and call boundaries, one ending on a closing slot
    (its last missing slot has B % 4 == 3), one after which the first burst is a closing one, and one channel silent for a
    whole call.  Returns a bool [S, T * calls] of missing slots and a description for the reach asserts."""
    Tt = T * calls
    miss = np.zeros((S, Tt), bool)
    gaps = []
    for s in range(S):
        if s % 5 == 4:
            continue                                           # some channels without a long gap
        g = int(rng.integers(3, 11)) * P + int(rng.integers(0, P))
        if s % 5 == 0:                                         # straddles a call boundary
            b = T * int(rng.integers(1, calls))
            lo = b - int(rng.integers(1, g))
        else:
            lo = int(rng.integers(0, Tt - g))
        miss[s, lo:lo + g] = True
        gaps.append((s, lo, lo + g))
    s0, s1, s2 = 1, 2, 3
    e0 = 4 * (T // 4 + 2)                                      # s0: missing up to and including closing slot e0 - 1
    e1 = 4 * (2 * T // 4 - 1) + 3                              # s1: the first burst after the gap is closing slot e1
    miss[s0] = False; miss[s0, e0 - 4 * P - 2:e0] = True
    miss[s1] = False; miss[s1, e1 - 5 * P - 1:e1] = True
    miss[s2] = False; miss[s2, 2 * T:3 * T] = True             # silent for the whole third call
    assert (e0 - 1) % 4 == 3 and e1 % 4 == 3
    gaps += [(s0, e0 - 4 * P - 2, e0), (s1, e1 - 5 * P - 1, e1), (s2, 2 * T, 3 * T)]
    return miss, gaps


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tch", [True, False])
@pytest.mark.parametrize("wire", [True, False])
def test_long_gaps_over_chained_calls_ragged(t, tx, prims, tch, wire):
    """255 channels x 9 blocks per call (2,295 code words: the last workgroup holds 3), five chained calls; every channel's
    bursts missing for 3 to 10 periods somewhere, so rx_source walks back over many periods, into earlier calls' state."""
    rng = np.random.default_rng(500 + 2 * tch + wire)
    S, n, calls = 255, 9, 5
    P, T = (8 if tch else 4), 4 * n
    assert (S * n) % 4 == 3
    rows, full = long_stream(rng, tx, prims.fo, tch, S, n * calls)
    miss, gaps = gap_plan(rng, S, T, calls, P)
    orig = full.copy()
    full[miss] = -1
    full[rng.random(full.shape) < 0.03] = -1
    (_, _, e0), (_, _, e1) = gaps[-3][:3], gaps[-2][:3]
    full[1, e0:e0 + 8] = orig[1, e0:e0 + 8]                    # the bursts right after the two marked gaps are present
    full[2, e1] = orig[2, e1]
    assert max(hi - lo for _, lo, hi in gaps) >= 10 * P and min(hi - lo for _, lo, hi in gaps) >= 3 * P
    assert any(lo // T != (hi - 1) // T for _, lo, hi in gaps)                          # a gap crossing a call boundary
    assert (full[3, 2 * T:3 * T] < 0).all() and (full[3, :2 * T] >= 0).any()
    b0 = rng.choice([0, 4], S).astype(np.uint8) if tch else None
    st = np.zeros((S, state_bytes(tch)), np.uint8)
    mst = st.copy()
    for c in range(calls):
        index = full[:, c * T:(c + 1) * T].astype(np.int32)
        bc = None if b0 is None else ((b0.astype(int) + c * T) % 8).astype(np.uint8)
        g = gpu_stream(t, tch, rows, index, st, b0=bc, wire=wire)
        m = fsm.run(prims, tch, rows, index, mst, b0=bc, wire=wire)
        same(g, m, ("call", c))
        st, mst = g["state"], m["state"]
        if c == 2:
            assert not m["status"][3].any()
    # the whole stream in one call decodes the same blocks (chaining is invisible)
    one = gpu_stream(t, tch, rows, full.astype(np.int32), np.zeros_like(st), b0=b0, wire=wire)
    assert np.array_equal(one["state"], st)


@pytest.mark.timeout(300)
def test_index_edges_and_a_large_soft_buffer(t, tx, prims):
    """Rows at the end of a soft buffer of more than 2^31 floats (soft_stride 164 > 148), so the row offsets only fit in
    size_t; indices -1, n_rows, n_rows - 1, INT32_MIN and INT32_MAX in one stream; TCH channels with b0 of 0, 4 and invalid
    values in the same call; and the XCCH decoder on the same buffer."""
    import torch
    stride, n_rows = 164, 13_200_000
    assert n_rows * stride > 2 ** 31
    rng = np.random.default_rng(600)
    S, n = 8, 8
    T = 4 * n
    soft, _, _ = fsm.tch_bursts(rng, tx, S, n, noise=0.35, p_junk=0.05)
    xsoft, _ = fsm.xcch_bursts(rng, prims.fo, S, n, noise=0.35)
    big = torch.empty((n_rows, stride), dtype=torch.float32, device="cuda")
    base = n_rows - 2 * S * T                                    # TCH rows then XCCH rows, up to the buffer's last row
    host = np.concatenate([soft.reshape(S * T, 148), xsoft.reshape(S * T, 148)])
    pad = rng.random((2 * S * T, stride)).astype(np.float32)
    pad[:, :148] = host
    big[base:].copy_(torch.from_numpy(pad))
    torch.cuda.synchronize()
    for tch in (True, False):
        index = (base + (0 if tch else S * T) + np.arange(S * T).reshape(S, T)).astype(np.int64)
        perm = rng.permutation(S)
        index = index[perm]
        index[rng.random((S, T)) < 0.1] = -1
        edges = [-1, n_rows, n_rows - 1, -2 ** 31, 2 ** 31 - 1]
        for s in range(S):
            for k, e in enumerate(edges):
                index[s, (3 + 5 * k + s) % T] = e
        index[0, 3::4] = n_rows - 1                               # closing bursts from the very last row
        index = index.astype(np.int32)
        b0 = np.array([0, 4, 2, 0, 4, 255, 1, 0], np.uint8) if tch else None
        st = np.zeros((S, state_bytes(tch)), np.uint8)
        st[:, fsm.HDR:] = rng.random((S, (state_bytes(tch) - fsm.HDR) // 4)).astype(np.float32).view(np.uint8)
        g = gpu_stream(t, tch, big, index, st, b0=b0)
        # the model on the rows the index reaches, renumbered (an index outside [0, n_rows) stays outside)
        used = np.unique(index[(index >= 0) & (index < n_rows)])
        rows = big[torch.from_numpy(used.astype(np.int64)).cuda()][:, :148].cpu().numpy()
        mi = np.full(index.shape, -1, np.int64)
        ok = (index >= 0) & (index < n_rows)
        mi[ok] = np.searchsorted(used, index[ok])
        m = fsm.run(prims, tch, rows, mi, st, b0=b0)
        same(g, m, ("edges", tch))
        assert (used >= base).all() and used.max() == n_rows - 1 and int(used.min()) * stride > 2 ** 31
        assert g["status"][0].all() and (g["status"][0] & fsm.DECODED).all()             # every block closed by row n_rows-1
        if tch:
            bad = np.isin(b0, (0, 4), invert=True)
            assert bad.any() and not g["status"][bad].any() and np.array_equal(g["state"][bad], st[bad])
            assert (g["status"][~bad] & fsm.DECODED).any()
    del big
    torch.cuda.empty_cache()


def test_host_refuses_the_kernels_block_limit(t):
    """k_fec_rx_stream numbers (channel, block) code words in an int and assumes n_chan * n_blocks < 2^29, i.e.
    n_chan * n_slots < 2^31: the host refuses every factoring that reaches it, before anything is launched."""
    L, h, EINVAL = t.L, t.h, -1
    fake = 256                                                      # never dereferenced: the call must fail on its sizes
    for n_chan, n_slots in ((2 ** 29, 4), (2 ** 27, 16), (2 ** 14, 2 ** 17), (3, 715827884),
                            (2, 2 ** 30), (2 ** 30, 2 ** 30 - 4), (2 ** 31 - 1, 4)):
        assert n_chan * n_slots >= 2 ** 31 and n_slots % 4 == 0, (n_chan, n_slots)
        for tch in (True, False):
            if tch:
                r = L.trxsig_fec_tch_decode_stream(h, n_chan, n_slots, fake, 148, 1, fake, None, 1, fake, fake, fake, fake, None)
            else:
                r = L.trxsig_fec_xcch_decode_stream(h, n_chan, n_slots, fake, 148, 1, fake, 1, fake, fake, fake, None)
            assert r == EINVAL, (tch, n_chan, n_slots)


@pytest.mark.timeout(600)
def test_just_under_the_block_limit(t, prims):
    """The largest kind of call the host accepts: 16,383 XCCH channels x 131,076 slots = 2^31 - 65,540 slots, 536,854,527
    code words (the last workgroup holds 3, its last code word's number is just under 2^29).  Three channels carry bursts
    (the first channel's first blocks, one in the middle, the last channel's last blocks, whose code words sit in the final
    workgroup); every other channel sees none.  Those three equal the model over their whole streams; every other channel
    reports nothing and keeps its state and FER."""
    import torch
    S, T = 16383, 131076
    nb = T // 4
    assert 2 ** 31 - 2 ** 17 < S * T < 2 ** 31 and (S * nb) % 4 == 3 and 2 ** 29 - S * nb < 2 ** 20
    rng = np.random.default_rng(700)
    xs, _ = fsm.xcch_bursts(rng, prims.fo, 3, 8, noise=0.35)
    rows = xs.reshape(96, 148)
    busy = {0: 0, S // 2: T // 2 + 1, S - 1: T - 32}              # channel -> first slot of its 32 bursts
    index = torch.full((S, T), -1, dtype=torch.int32, device="cuda")
    hidx = {}
    for k, (ch, lo) in enumerate(busy.items()):
        h = np.full(T, -1, np.int32)
        h[lo:lo + 32] = 32 * k + np.arange(32)
        h[lo + rng.choice(32, 3, replace=False)] = -1
        index[ch] = torch.from_numpy(h).cuda()
        hidx[ch] = h
    st0 = rng.random((S, fsm.XCCH_STATE_BYTES // 4)).astype(np.float32).view(np.uint8)
    st0[:, 4:fsm.HDR] = 0
    st = dev(st0)
    status = torch.full((S, nb), 0xEE, dtype=torch.uint8, device="cuda")
    l2 = torch.full((S, nb, 23), 0xEE, dtype=torch.uint8, device="cuda")
    fer = torch.full((S, nb), float("nan"), dtype=torch.float32, device="cuda")
    t.fec_xcch_decode_stream(dev(rows), index, st, status, l2, fer=fer)
    torch.cuda.synchronize()
    del index
    quiet = torch.ones(S, dtype=torch.bool, device="cuda")
    quiet[list(busy)] = False
    assert int(status.amax(dim=1)[quiet].max()) == 0
    assert int(l2.view(S, nb * 23).amax(dim=1)[quiet].max()) == 0
    fer0 = torch.from_numpy(st0[:, :4].copy().view(np.float32)).cuda()
    assert bool((fer.view(torch.int32) == fer0.view(torch.int32)).all(dim=1)[quiet].all())
    gst = st.cpu().numpy()
    q = quiet.cpu().numpy()
    assert np.array_equal(gst[q], st0[q])
    for ch, h in hidx.items():
        m = fsm.run(prims, False, rows, h.reshape(1, T), st0[ch:ch + 1])
        g = dict(status=status[ch:ch + 1].cpu().numpy(), l2=l2[ch:ch + 1].cpu().numpy(), fer=fer[ch:ch + 1].cpu().numpy(),
                 state=gst[ch:ch + 1])
        same(g, m, ("busy channel", ch))
        assert (m["status"] & fsm.DECODED).sum() >= 5
    del status, l2, fer
    torch.cuda.empty_cache()
