"""GPU parity of packet access through L1 (trxsig_l1pacc) against tests/l1_pacc_model.py: the handset side's grid byte for byte
(own grid, overlay, splits, the hyperframe wrap); the base-station side equal to the model in every output and in the table on
the closed-loop cells that tests/test_l1_pacc_model.py runs on the CPU (sps 1 and 4), on a noisy set and on a set with empty
occasions, on both legs, whole and split; the timing-advance loop on the card; the refusals last.

What the model is made of per leg.  TRXSIG_RACHLEG_DEMOD: the oracle's detectRACHBurst and demodulateBurst on the card's cells,
copied to the host.  TRXSIG_RACHLEG_MLSE: the detector's flags, amplitudes and arrival times are the oracle's too; the soft rows
are trxsig_mlse_rach_batch's from a direct call on the same occasion list (that equaliser has its own model and tests).  avgPwr,
which the oracle's batch call does not return, is held against trxsig_detect_demod_rach_batch's on the same list."""
import numpy as np
import pytest

import _pkg
import fecbind
import l1_pacc_model as lp
import oraclebind

pytestmark = pytest.mark.gpu

HYPER = lp.HYPERFRAME
COMB, BSIC = lp.COMB, lp.BSIC
N = len(lp.pdchs(COMB))
KEYS = ("kind", "tai", "det", "fmt", "ok", "ra", "amp", "toa", "ta")


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def ctxs(pkg):
    out = {}
    for sps in (1, 4):
        out[sps] = pkg.TrxSig(sps, 0)
        out[sps].use_torch_stream()
    return out


@pytest.fixture(scope="module")
def fo():
    return fecbind.FecOracle()


def dev(a):
    import torch
    a = np.array(a, order="C")
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def gpu_encode(obj, fn, F, s, fmt, onto=None):
    import torch
    b, w = (None, None) if onto is None else onto
    obj.encode(fn, F, dev(s["ptcch_kind"]), dev(s["ptcch_ra"]), dev(s["prach_kind"]), dev(s["prach_ra"]), fmt=fmt, bits_onto=b, what_onto=w)
    torch.cuda.synchronize()
    g = obj.collect()
    return g["bits"], g["what"]


def model_encode(fo, fn, F, s, fmt, onto=None):
    return lp.encode(fo, COMB, BSIC, fn, F, s["ptcch_kind"], s["ptcch_ra"], s["prach_kind"], s["prach_ra"], fmt, onto)


@pytest.mark.parametrize("fn", [0, 403, HYPER - 40])
def test_encode_equals_model(pkg, ctxs, fo, fn):
    F = 130
    obj = pkg.L1Pacc(ctxs[4], COMB, BSIC)
    assert obj.channels() == N and [obj.channel(g) for g in range(N)] == lp.pdchs(COMB)
    assert obj.grid(fn, F) == lp.blocks(fn, F)[1]
    for fmt in (0, 1):
        s = lp.scenario(20 + fmt, fn, F, fmt)
        s["ptcch_ra"][0, :3] = (256, 2048, 65535)             # words that do not fit: not sent
        s["ptcch_kind"][0, :3] = 1
        s["ptcch_kind"][1, 5] = 2                             # another kind: not sent
        bits, what = gpu_encode(obj, fn, F, s, fmt)
        wb, ww = model_encode(fo, fn, F, s, fmt)
        assert np.array_equal(what, ww) and np.array_equal(bits, wb)
        assert (what == lp.W_PACC).sum() > 30 and set(np.unique(what)) == {0, lp.W_PACC}
    obj.destroy()


def test_overlay_touches_only_its_own_slots(pkg, ctxs, fo):
    import torch
    fn, F, A = 403, 130, COMB.shape[0]
    obj = pkg.L1Pacc(ctxs[4], COMB, BSIC)
    s = lp.scenario(23, fn, F, 1)
    rng = np.random.default_rng(5)
    b0, w0 = rng.integers(0, 2, (A, 8 * F, 148)).astype(np.uint8), rng.integers(1, 8, (A, 8 * F)).astype(np.uint8)
    raw_b, raw_w = torch.full((A * 8 * F * 148 + 65,), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((A * 8 * F + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    db, dw = raw_b[1:1 + b0.size], raw_w[:w0.size]            # a misaligned grid: the byte-store form
    db.copy_(dev(b0).view(-1)); dw.copy_(dev(w0).view(-1))
    obj.encode(fn, F, dev(s["ptcch_kind"]), dev(s["ptcch_ra"]), dev(s["prach_kind"]), dev(s["prach_ra"]), fmt=1, bits_onto=db, what_onto=dw)
    torch.cuda.synchronize()
    wb, ww = model_encode(fo, fn, F, s, 1, onto=(b0, w0))
    assert np.array_equal(db.cpu().numpy().reshape(b0.shape), wb) and np.array_equal(dw.cpu().numpy().reshape(w0.shape), ww)
    assert (raw_b.cpu().numpy()[[0] + list(range(1 + b0.size, raw_b.numel()))] == 0xA5).all() and (raw_w.cpu().numpy()[w0.size:] == 0xA5).all()
    assert (ww == lp.W_PACC).sum() > 30 and (ww != lp.W_PACC).sum() > 1000
    obj.destroy()


def pieces(fn, F, cuts):
    return [((fn + a) % HYPER, a, b - a) for a, b in zip((0,) + cuts, cuts + (F,))]


def piece_blocks(fn, F, a, Fp):
    """(first block of the piece relative to the call's, its count)"""
    blk0 = lp.blocks(fn, F)[0]
    ks = [k for k in range(Fp) if lp.block_of(fn + a + k)[0] >= 0]
    return (lp.block_of(fn + a + ks[0])[0] - blk0 if ks else 0), lp.blocks(fn + a, Fp)[1]


@pytest.mark.parametrize("fn", [403, HYPER - 40])
def test_encode_splits_equal_the_whole(pkg, ctxs, fo, fn):
    F, cuts = 130, (1, 13, 52, 77)
    obj = pkg.L1Pacc(ctxs[4], COMB, BSIC)
    s = lp.scenario(24, fn, F, 0)
    bits, what = gpu_encode(obj, fn, F, s, 0)
    pb, pw = [], []
    for pfn, a, Fp in pieces(fn, F, cuts):
        j0, nbp = piece_blocks(fn, F, a, Fp)
        assert obj.grid(pfn, Fp) == nbp
        sp = dict(s, prach_kind=np.ascontiguousarray(s["prach_kind"][:, j0:j0 + nbp]), prach_ra=np.ascontiguousarray(s["prach_ra"][:, j0:j0 + nbp]))
        b, w = gpu_encode(obj, pfn, Fp, sp, 0)
        pb.append(b); pw.append(w)
    assert np.array_equal(np.concatenate(pw, axis=1), what) and np.array_equal(np.concatenate(pb, axis=1), bits)
    obj.destroy()


def radiate(pkg, ctx, obj, s, fn, F, fmt):
    """The handsets' bursts of a call onto slot cells, on the card: encode -> trxsig_modulate_batch -> trxsig_delay_vector_batch
    -> trxsig_scale_vector_batch.  -> (cells as a float32 [.., 2] tensor, slot_stride, arfcn_stride)"""
    import torch
    sps, A, T = ctx.sps, COMB.shape[0], 8 * F
    cell = lp.CELL_SYMBOLS * sps
    out = obj.encode(fn, F, dev(s["ptcch_kind"]), dev(s["ptcch_ra"]), dev(s["prach_kind"]), dev(s["prach_ra"]), fmt=fmt)
    ch = lp.pdchs(COMB)
    sent = lp.sent_bursts(s, fn, F)
    B = len(sent)
    slot = np.array([8 * k + ch[g][1] for g, k, _, _ in sent], np.int64)
    arf = np.array([ch[g][0] for g, _, _, _ in sent], np.int64)
    bits = pkg._dev_tensor(ctx, out.d_bits, (A * T, 148), "|u1")[dev(arf * T + slot)].contiguous()
    off = dev(((slot * A + arf) * cell).astype(np.int32))
    guard = dev((8 + (slot % 4 == 0)).astype(np.int32))
    length = dev(((156 + (slot % 4 == 0)) * sps).astype(np.int32))
    tmp = torch.zeros(T * A * cell, 2, dtype=torch.float32, device="cuda")
    x = torch.zeros_like(tmp)
    ctx.modulate(bits, guard, tmp, off)
    L = pkg.lib()
    delay = dev(np.array([np.float32(d) * np.float32(sps) for _, _, _, d in sent], np.float32))
    assert L.trxsig_delay_vector_batch(ctx.h, tmp.data_ptr(), off.data_ptr(), length.data_ptr(), B, delay.data_ptr(), 0, x.data_ptr()) == 0
    scale = dev(np.tile(np.array([lp.AMPLITUDE, 0.0], np.float32), (B, 1)))
    assert L.trxsig_scale_vector_batch(ctx.h, x.data_ptr(), off.data_ptr(), length.data_ptr(), B, 157 * sps, scale.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    return x, A * cell, cell


def direct(pkg, ctx, x, occ, leg):
    """trxsig_detect_demod_rach_batch / trxsig_mlse_rach_batch called directly on an occasion list: (avgpwr, soft) on the host."""
    import torch
    B = len(occ)
    off, length = dev(np.array([o[3] for o in occ], np.int32)), dev(np.array([o[4] for o in occ], np.int32))
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = torch.zeros(B, 2, device="cuda"); toa = torch.zeros(B, device="cuda")
    pwr = torch.zeros(B, device="cuda"); soft = torch.zeros(B, 148, device="cuda")
    call = ctx.mlse_rach if leg else ctx.detect_demod_rach
    call(x, off, length, flags, amp, toa, soft, avgpwr=pwr, detect_thresh=5.0, energy_thresh=-1.0)
    torch.cuda.synchronize()
    return pwr.cpu().numpy(), soft.cpu().numpy()


def check_detect(pkg, ctx, fo, so, x, ss, sa, fn, F, prach, fmt, cuts, wire=True):
    """detect on both legs, whole and split at cuts, against the model in every output and in the table."""
    import torch
    host = np.ascontiguousarray(x.cpu().numpy()).view(np.complex64).ravel()
    occ = lp.cell_list(COMB, fn, F, prach, ctx.sps, ss, sa)
    ok, amp, toa, soft_d = so.rach_batch(host, [o[3] for o in occ], [o[4] for o in occ], thresh=5.0, nthreads=4)
    last = None
    for leg in (pkg.RACHLEG_DEMOD, pkg.RACHLEG_MLSE):
        pwr, soft_g = direct(pkg, ctx, x, occ, leg)
        soft = soft_g if leg else soft_d
        if not leg:
            assert np.array_equal(soft_g, soft_d), "the card's demodulator and the oracle's differ on these cells"
        mt = lp.Table(N)
        want = lp.fold(fo, mt, COMB, BSIC, fn, F, prach, ctx.sps, occ, ok, amp, toa, pwr, soft, fmt, wire)
        for split in (False, True):
            obj = pkg.L1Pacc(ctx, COMB, BSIC)
            got = []
            for pfn, a, Fp in (pieces(fn, F, cuts) if split else [(fn, 0, F)]):
                j0, nbp = piece_blocks(fn, F, a, Fp)
                pp = None if prach is None else np.ascontiguousarray(prach[:, j0:j0 + nbp])
                obj.detect(x.data_ptr() + 8 * (8 * a * ss), ss, sa, pfn, Fp, prach=pp, fmt=fmt, leg=leg, wire=wire)
                got.append(obj.collect())
            for key in KEYS + ("avgpwr",):
                g = np.concatenate([p[key] for p in got], axis=1)
                w = want[key] if key != "amp" else want[key].view(np.float32).reshape(N, F, 2)
                assert np.array_equal(g, w), (leg, split, key, np.argwhere(g != w)[:6])
            assert mt.same(obj.states()), (leg, split)
            obj.destroy()
        last = want
    return last, mt


@pytest.mark.parametrize("sps", [1, 4])
def test_detect_on_the_closed_loop_cells(pkg, ctxs, fo, sps):
    """The CPU test's inputs (same seed, plan, words, delays, level; no noise), radiated on the card: equal to the model, and
    every burst sent comes back detected and ok with its word and TA = round(delay); a marked block that the handsets left
    empty gives det == 0 rows."""
    fn, F, ctx = 403, 130, ctxs[sps]
    so = oraclebind.Oracle(sps)
    for fmt in (0, 1):
        s = lp.scenario(11, fn, F, fmt)
        ms = pkg.L1Pacc(ctx, COMB, BSIC)
        x, ss, sa = radiate(pkg, ctx, ms, s, fn, F, fmt)
        r, t = check_detect(pkg, ctx, fo, so, x, ss, sa, fn, F, s["prach"], fmt, (1, 13, 52, 77))
        sent = lp.sent_bursts(s, fn, F)
        for g, k, ra, delay in sent:
            assert (r["det"][g, k], r["ok"][g, k], r["fmt"][g, k], r["ra"][g, k], r["ta"][g, k]) == (1, 1, fmt, ra, int(np.floor(delay + 0.5)))
        here = {(g, k) for g, k, _, _ in sent}
        empty = [(g, k) for g in range(N) for k in range(F) if r["kind"][g, k] == lp.PRACH and (g, k) not in here]
        assert len(empty) >= 8 and not any(r["det"][g, k] for g, k in empty)
        ms.destroy()


def test_detect_with_noise_either_format_and_empty_occasions(pkg, ctxs, fo):
    """15 dB (seeded), fmt -1, across the hyperframe wrap; then a call whose occasions are all empty, and one without marks."""
    import torch
    fn, F, ctx = HYPER - 40, 130, ctxs[4]
    so = oraclebind.Oracle(4)
    s = lp.scenario(31, fn, F, 1)
    ms = pkg.L1Pacc(ctx, COMB, BSIC)
    x, ss, sa = radiate(pkg, ctx, ms, s, fn, F, 1)
    g = torch.Generator(device="cuda"); g.manual_seed(32)
    sigma = lp.AMPLITUDE / np.sqrt(2.0 * 10.0 ** 1.5)
    x += sigma * torch.randn(x.shape, device="cuda", generator=g)
    r, t = check_detect(pkg, ctx, fo, so, x, ss, sa, fn, F, s["prach"], -1, (1, 39, 40, 41, 100))
    assert r["ok"].sum() >= 15 and t.valid.sum() >= 5
    check_detect(pkg, ctx, fo, so, x, ss, sa, fn, F, s["prach"], 1, (77,), wire=False)
    x.zero_()
    x += 3.0 * torch.randn(x.shape, device="cuda", generator=g)
    r, t = check_detect(pkg, ctx, fo, so, x, ss, sa, fn, F, s["prach"], -1, (13,))
    assert (r["kind"] != 0).sum() > 40 and not r["ok"].any() and not t.valid.any()
    r, _ = check_detect(pkg, ctx, fo, so, x, ss, sa, fn, F, None, 0, (52,))
    assert not (r["kind"] == lp.PRACH).any() and (r["kind"] == lp.PTCCH).sum() == N * sum(lp.tai_of(fn + k) >= 0 for k in range(F))
    ms.destroy()


def loop_result(pkg, ctx, out, A, F):
    """A trxsig_l1pdch_encode grid as the pull a handset would have made of it: the bits as soft values, every written slot a row."""
    import torch
    T = 8 * F
    what = pkg._dev_tensor(ctx, out.d_what, (A, T), "|u1")
    row = torch.where(what.t() != 0, (torch.arange(A, device="cuda")[None, :] * T + torch.arange(T, device="cuda")[:, None]).to(torch.int32),
                      torch.tensor(-1, dtype=torch.int32, device="cuda")).contiguous()
    keep = dict(row=row, valid=torch.full((A * T,), 2, dtype=torch.uint8, device="cuda"), amp=torch.ones(A * T, 2, device="cuda"),
                toa=torch.zeros(A * T, device="cuda"), soft=pkg._dev_tensor(ctx, out.d_bits, (A * T, 148), "|u1").to(torch.float32).contiguous())
    res = pkg.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=A * T, d_row=row.data_ptr(), d_valid=keep["valid"].data_ptr(), d_flags=None,
                             d_amp=keep["amp"].data_ptr(), d_toa=keep["toa"].data_ptr(), d_avgpwr=None, d_threshold=None,
                             d_soft=keep["soft"].data_ptr(), soft_stride=148)
    return res, keep


def test_the_timing_advance_loop_on_the_card(pkg, ctxs, fo):
    """handset encode -> modulate / delay / scale -> cells -> detect -> ta_message -> L1Pdch(DOWN).encode -> bits as soft values ->
    L1Pdch(DOWN).decode -> ta_read: round(delay) for every TAI that sent, every other TAI unchanged; after the handsets' delays
    change, the next 416 frames give the new values."""
    import torch
    ctx, A, F = ctxs[4], COMB.shape[0], 416
    ms, bts = pkg.L1Pacc(ctx, COMB, BSIC), pkg.L1Pacc(ctx, COMB, BSIC)
    down, hs = pkg.L1Pdch(ctx, COMB, BSIC, pkg.L1PDCH_DOWN), pkg.L1Pdch(ctx, COMB, BSIC, pkg.L1PDCH_DOWN)
    ta = torch.full((N, 16), 99, dtype=torch.uint8, device="cuda")
    s = lp.scenario(41, 0, F, 0, p_prach=0.0)
    assert 0 < s["ptcch_kind"].sum() < N * 16
    want = np.full((N, 16), 99, np.uint8)
    for rnd, fn in enumerate((0, 416)):
        if rnd:
            s["ptcch_delay"] = lp.delays(np.random.default_rng(42), (N, 16))
        x, ss, sa = radiate(pkg, ctx, ms, s, fn, F, 0)
        bts.detect(x, ss, sa, fn, F, prach=None, fmt=0)
        F2, fn2 = 104, fn + F
        nb_pd, nb_pt = down.grid(fn2, F2)
        kind, payload = torch.zeros(N, nb_pt, dtype=torch.uint8, device="cuda"), torch.zeros(N, nb_pt, 23, dtype=torch.uint8, device="cuda")
        bts.ta_message(kind, payload, nb_pt)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device="cuda")
        out = down.encode(fn2, F2, z(N, nb_pd), z(N, nb_pd), z(N, nb_pd, 54), kind, payload)
        res, keep = loop_result(pkg, ctx, out, A, F2)
        dec = hs.decode(res, fn2, wire=True, cs_force=0)
        ms.ta_read(dec, ta)
        torch.cuda.synchronize()
        sent = s["ptcch_kind"] == 1
        want = np.where(sent, np.floor(s["ptcch_delay"] + 0.5).astype(np.uint8), want)
        assert np.array_equal(ta.cpu().numpy(), want), rnd
        assert np.array_equal(payload.cpu().numpy()[:, 0, :16], np.where(sent, want, 0x7F)) and (payload.cpu().numpy()[:, :, 16:] == 0x2B).all()
        st = bts.states()
        assert np.array_equal(st["valid"] != 0, sent) and (st["fn"][sent] >= fn).all() and (st["fn"][sent] < fn + F).all()
    assert (want[~sent] == 99).all() and (want[sent] <= 20).all()
    for o in (ms, bts, down, hs):
        o.destroy()


# ---- the refusals, last ----
def test_refusals(pkg, ctxs):
    import ctypes as C
    import torch
    ctx = ctxs[4]
    L = pkg.lib()
    h = C.c_void_p()
    comb = np.ascontiguousarray(COMB)
    create = lambda n, cb, bsic: L.trxsig_l1pacc_create(C.byref(h), ctx.h, n, cb.ctypes.data if cb is not None else None, bsic)
    bad = comb.copy(); bad[0, 2] = 2
    for args in ((0, comb, 5), (2, None, 5), (2, comb, 64), (2, comb, -1), (2, bad, 5)):
        assert create(*args) == -1 and not h.value
    assert b"trxsig_l1pacc_create" in L.trxsig_last_error(ctx.h)
    obj = pkg.L1Pacc(ctx, COMB, BSIC)
    s = lp.scenario(1, 0, 52, 0)
    a = lambda: (dev(s["ptcch_kind"]), dev(s["ptcch_ra"]), dev(s["prach_kind"]), dev(s["prach_ra"]))
    b = torch.zeros(2 * 8 * 52 * 148, dtype=torch.uint8, device="cuda")
    for fn, F, kw in ((-1, 52, {}), (HYPER, 52, {}), (0, 0, {}), (0, 52, dict(fmt=2)), (0, 52, dict(fmt=-1)), (0, 52, dict(bits_onto=b))):
        with pytest.raises(pkg.TrxSigError, match="trxsig_l1pacc_encode"):
            obj.encode(fn, F, *a(), **kw)
    with pytest.raises(pkg.TrxSigError, match="trxsig_l1pacc_encode"):
        obj.encode(0, 52, None, *a()[1:])
    x = torch.zeros(8 * 52 * 2 * 640, 2, device="cuda")
    for fn, F, kw in ((-1, 52, {}), (0, 0, {}), (0, 52, dict(fmt=2)), (0, 52, dict(fmt=-2)), (0, 52, dict(leg=2))):
        with pytest.raises(pkg.TrxSigError, match="trxsig_l1pacc_detect"):
            obj.detect(x, 1280, 640, fn, F, **kw)
    with pytest.raises(pkg.TrxSigError, match="int32"):
        obj.detect(x, 1 << 26, 640, 0, 52)                   # an occasion's offset past 2^31 samples
    with pytest.raises(pkg.TrxSigError, match="int32"):
        obj.detect(x, -1280, 640, 0, 52)
    with pytest.raises(pkg.TrxSigError, match="trxsig_l1pacc_detect"):
        obj.detect(None, 1280, 640, 0, 52)
    with pytest.raises(pkg.TrxSigError, match="trxsig_l1pacc_ta_message"):
        obj.ta_message(None, None, 2)
    with pytest.raises(pkg.TrxSigError, match="trxsig_l1pacc_ta_message"):
        obj.ta_message(b, b, -1)
    obj.ta_message(None, None, 0)
    up = pkg.L1Pdch(ctx, COMB, BSIC, pkg.L1PDCH_UP)           # an UP object has no PTCCH class: not a handset's decode
    row = torch.full((32, 2), -1, dtype=torch.int32, device="cuda")
    res = pkg.TrxGroupResult(n_slots=32, n_arfcn=2, n_rows=0, d_row=row.data_ptr(), d_valid=None, d_flags=None, d_amp=None, d_toa=None,
                             d_avgpwr=None, d_threshold=None, d_soft=None, soft_stride=148)
    dec = up.decode(res, 0)
    with pytest.raises(pkg.TrxSigError, match="trxsig_l1pacc_ta_read"):
        obj.ta_read(dec, b)
    assert L.trxsig_l1pacc_ta_read(obj.h, None, b.data_ptr()) == -1 and L.trxsig_l1pacc_grid(obj.h, 0, 0, None) == -1
    assert L.trxsig_l1pacc_channel(obj.h, N, None, None) == -1 and L.trxsig_l1pacc_state(obj.h, None) == -1
    ctx.synchronize()
    obj.destroy(); up.destroy()
