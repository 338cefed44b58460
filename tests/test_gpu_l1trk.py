"""GPU tests of the tracking receiver (include/trxsig_l1trk.h) against tests/l1_trk_model.py, at sps 1, 2 and 4.

  slice         3 columns on 2 phones, 2 frames, guard words round every cell and NaN round every stream: raw words equal to the
                model; steps zero and not, a phase and a distance * step that wrap past 2^32, a span that starts before the
                buffer and one that runs past its end (zeros, the clipped bit, nothing read outside), an unlocked phone, both
                stride nestings, anchors behind and ahead of the call and across the hyperframe's wrap, one call equal to two
  FCCH records  C and E within 4 2^-24 sum |y[n + sps]| |y[n]| (4 2^-24 E) of float64, the acceptance flags on a tone and on noise
  update        results the test builds: pos, phase, quiet and the sums exactly the model's, step within the stated bound,
                d_use given and NULL
  refusals      the argument rules that need a live object, and the context kept alive
  closed loop   L1Tx -> modulate -> Air.stream -> L1Acq.search -> seed, six rounds of stream -> slice -> TrxGroup.pull -> update
                -> L1MsRx.decode with both clocks drifting: the truth conditions tests/test_l1_trk_model.py holds the model to"""
import ctypes as C

import numpy as np
import pytest

import _pkg
import l1_trk_model as ltm
import oraclebind

pytestmark = pytest.mark.gpu
EINVAL = -1
HYPER = ltm.HYPER
GUARD = np.complex64(complex(-777.25, 123.5))
PHONE, C0 = [0, 0, 1], [0, 2]


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
    """where cell (c, t) lies in a flat buffer: `lead` samples, then cells of 157 sps + gap in either nesting"""

    def __init__(self, A, T, sps, nest, gap=3, lead=5):
        self.A, self.T, self.sps, self.lead = A, T, sps, lead
        cell = 157 * sps + gap
        self.slot, self.col = (cell, T * cell) if nest == "col-major" else (A * cell, cell)
        self.total = lead + A * T * cell

    def at(self, c, t):
        return self.lead + t * self.slot + c * self.col

    def pack(self, cells):
        buf = np.full(self.total, GUARD, np.complex64)
        for c in range(self.A):
            for t in range(self.T):
                buf[self.at(c, t):self.at(c, t) + len(cells[c][t])] = cells[c][t]
        return buf


class Rig:
    def __init__(self, pkg, sps):
        self.pkg, self.sps = pkg, sps
        self.ctx = pkg.TrxSig(sps, 0)
        self.ctx.use_torch_stream()
        self.o = oraclebind.Oracle(sps)

    def pair(self, max_frames=2, phone=PHONE, c0=C0, **kw):
        return self.pkg.L1Trk(self.ctx, phone, c0, max_frames, **kw), ltm.TrkModel(self.o, phone, c0, **kw)

    def slice(self, trk, model, x, n0, fn, F, nest="col-major"):
        """x [n_cols][n_samples] on both; the device's buffers carry NaN round every stream and guard words round every cell.
        Asserts words, guards, status and anchors; returns (the device's collect(), the model's records)."""
        n_cols, n = x.shape
        stride, lead = n + 9, 4
        buf = np.full(lead + n_cols * stride, np.complex64(complex(np.nan, np.nan)), np.complex64)
        for c in range(n_cols):
            buf[lead + c * stride:lead + c * stride + n] = x[c]
        d_x = dev(buf.view(np.float32))
        lay = Layout(n_cols, 8 * F, self.sps, nest)
        d_cells = dev(np.full(lay.total, GUARD, np.complex64).view(np.float32))
        trk.slice(d_x.data_ptr() + 8 * lead, stride, n0, n, fn, F, d_cells.data_ptr() + 8 * lay.lead, lay.slot, lay.col)
        cells, status, rec = model.slice(x, n0, fn, F)
        g = trk.collect()
        got = d_cells.cpu().numpy().view(np.complex64).ravel()
        want = lay.pack(cells)
        bad = np.argwhere(words(got) != words(want))
        assert not len(bad), ("cells differ from the model (or a guard word was written)", bad[:4], got[bad[:4, 0]], want[bad[:4, 0]])
        assert np.array_equal(d_x.cpu().numpy().view(np.uint32), buf.view(np.float32).view(np.uint32)), "the streams were written"
        assert list(g["status"]) == status
        same_state(g, model)
        return g, rec


def same_state(g, model):
    lk = np.array(model.locked, bool)
    assert list(g["locked"]) == model.locked and list(g["quiet"]) == model.quiet
    for key in ("fn", "pos", "phase", "step"):
        assert [int(v) for v in g[key]] == getattr(model, key), (key, g[key], getattr(model, key), lk)


@pytest.fixture(scope="module", params=[1, 2, 4])
def rig(request, pkg):
    r = Rig(pkg, request.param)
    yield r
    r.ctx.close()


def noise(rng, shape, amp=1.0):
    return (amp * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(np.complex64)


def set_both(trk, model, p, *a):
    trk.set(p, *a); model.set(p, *a)


def test_slice_words(rig):
    sps = rig.sps
    rng = np.random.default_rng(100 + sps)
    frame, F = 1250 * sps, 2
    n = F * frame + 40
    x = noise(rng, (3, n))
    fn = 51 * 1000 + 7
    # step 0 and not, inside the buffer; col-major
    trk, m = rig.pair()
    set_both(trk, m, 0, 1, fn, 10 ** 7 + 11, 0, 0x12345678)
    set_both(trk, m, 1, 1, fn, 10 ** 7 + 40, 0x00abcdef, 0)
    g, _ = rig.slice(trk, m, x, 10 ** 7, fn, F)
    assert list(g["status"]) == [0, 0, 0]
    # the anchors now stand at fn + 2: a second call goes on from them (slot-major), the phase of phone 1 has advanced
    g, _ = rig.slice(trk, m, noise(rng, (3, n)), 10 ** 7 + F * frame, fn + F, F, "slot-major")
    assert list(g["status"]) == [0, 0, 0] and list(g["fn"]) == [fn + 2 * F] * 2
    trk.destroy()
    # a phase and a distance * step that wrap past 2^32: anchors 7 frames behind and 3 ahead of the call
    trk, m = rig.pair()
    set_both(trk, m, 0, 1, fn - 7, 5 * 10 ** 9 - 7 * frame, 0x87654321, 0xfffffff0)
    set_both(trk, m, 1, 1, fn + 3, 5 * 10 ** 9 + 3 * frame + 33, 0xfedcba98, 0x80000000)
    g, _ = rig.slice(trk, m, x, 5 * 10 ** 9, fn, F, "slot-major")
    assert list(g["status"]) == [0, 0, 0] and list(g["pos"]) == [5 * 10 ** 9 + F * frame, 5 * 10 ** 9 + F * frame + 33]
    trk.destroy()
    # across the hyperframe's wrap, both ways: anchor 1 and call HYPER - 1 (distance -2); anchor HYPER - 3 and call HYPER - 1
    trk, m = rig.pair()
    set_both(trk, m, 0, 1, 1, 2 * frame + 3, 0x0badf00d, 7)
    set_both(trk, m, 1, 1, HYPER - 3, 20 - 2 * frame, 0xf0000001, 9)
    g, _ = rig.slice(trk, m, x, 0, HYPER - 1, F)
    assert list(g["status"]) == [0, 0, 0] and list(g["fn"]) == [1, 1] and list(g["pos"]) == [3 + F * frame, 20 + F * frame]
    trk.destroy()


def test_slice_edges(rig):
    sps = rig.sps
    rng = np.random.default_rng(200 + sps)
    frame, F = 1250 * sps, 2
    n = F * frame - 50                                         # shorter than the span
    x = noise(rng, (3, n))
    fn = 777
    # phone 0 starts 30 samples before the buffer (and runs 20 past its end); phone 1 starts inside and runs 70 past its end
    trk, m = rig.pair()
    set_both(trk, m, 0, 1, fn, 1000 - 30, 0x01020304, 1)
    set_both(trk, m, 1, 1, fn, 1000 + 20, 0x7fffffff, 2)
    g, _ = rig.slice(trk, m, x, 1000, fn, F, "slot-major")
    assert list(g["status"]) == [ltm.CLIPPED] * 3
    trk.destroy()
    # wholly outside the buffer (before it, after it): zeros everywhere; an unlocked phone: zeros and its own bit, anchor untouched
    trk, m = rig.pair()
    set_both(trk, m, 0, 1, fn, -10 ** 12, 5, 5)
    set_both(trk, m, 1, 0, fn - 1, 1000, 0x01020304, 3)
    g, _ = rig.slice(trk, m, x, 1000, fn, F)
    assert list(g["status"]) == [ltm.CLIPPED, ltm.CLIPPED, ltm.UNLOCKED] and list(g["fn"]) == [fn + F, fn - 1]
    set_both(trk, m, 0, 1, fn, 10 ** 12, 5, 5)
    rig.slice(trk, m, x, 1000, fn, F)
    trk.destroy()


def test_one_call_equals_two(rig):
    sps = rig.sps
    rng = np.random.default_rng(300 + sps)
    frame = 1250 * sps
    n = 2 * frame + 64
    x = noise(rng, (3, n))
    fn = 51 * 9 + 9                                            # the second frame is an FCCH frame
    start = lambda: ((0, 1, fn - 1, 40 - frame, 0x13579bdf, 0xffff0000), (1, 1, fn, 12, 0xeca86420, 0x0000ffff))
    whole, mw = rig.pair()
    for a in start():
        set_both(whole, mw, *a)
    gw, _ = rig.slice(whole, mw, x, 0, fn, 2)
    parts, mp = rig.pair()
    for a in start():
        set_both(parts, mp, *a)
    rig.slice(parts, mp, x, 0, fn, 1)                          # (each call is held to the model, which holds split = whole)
    gp, _ = rig.slice(parts, mp, x, 0, fn + 1, 1)
    for key in ("fn", "pos", "phase", "step"):
        assert np.array_equal(gw[key], gp[key]), key
    assert gw["n_fcch"] == gp["n_fcch"] == 1 and np.array_equal(gw["fcch_fn"], gp["fcch_fn"]) and list(gw["fcch_fn"][:, 0]) == [fn + 1] * 2
    assert np.array_equal(gw["fcch_c"], gp["fcch_c"]) and np.array_equal(gw["fcch_e"], gp["fcch_e"])
    whole.destroy(); parts.destroy()


def fcch_case(rig, F=12):
    """12 frames from a frame with FN % 51 == 0 (FCCH frames 0 and 10: the records' capacity for max_frames 12 is exactly 2).
    Phone 0's C0 column hears a tone of a quarter turn per symbol and a little more, rotated so that its NCO brings it back; phone 1's hears
    noise."""
    sps = rig.sps
    rng = np.random.default_rng(400 + sps)
    frame = 1250 * sps
    n = F * frame + 32
    fn = 51 * 321
    x = noise(rng, (3, n), 0.05)
    step = 0x02345678
    k = np.arange(n, dtype=np.float64)
    tone = 3.0 * np.exp(2j * np.pi * (k * (0.25 + 0.003) / sps - k * step / 2.0 ** 32))    # a residual of 3e-3 cycle / symbol
    x[0] = (x[0] + tone).astype(np.complex64)
    trk, m = rig.pair(max_frames=F, afc_shift=2)
    set_both(trk, m, 0, 1, fn, 16, step, 0)
    set_both(trk, m, 1, 1, fn, 7, 0xff000000, 5)
    return trk, m, x, fn, F


def check_records(g, rec):
    for p in range(len(rec)):
        assert g["n_fcch"] == len(rec[p]) == 2
        for j, r in enumerate(rec[p]):
            assert int(g["fcch_fn"][p, j]) == r["fn"]
            dc, de = abs(complex(g["fcch_c"][p, j]) - r["C"]), abs(float(g["fcch_e"][p, j]) - r["E"])
            print("phone %d record %d: |dC| %.3e (bound %.3e) |dE| %.3e (bound %.3e) ok %d" % (p, j, dc, r["bound_c"], de, r["bound_e"], r["ok"]))
            assert dc <= r["bound_c"] and de <= r["bound_e"] and bool(g["fcch_ok"][p, j]) == r["ok"]
    good = [r for r in rec[0] if r["ok"]]                      # the bound on the AFC's sum, relative: sum of the bounds / |sum C|
    return sum(r["bound_c"] for r in good) / abs(sum(r["C"] for r in good)) if good else 0.0


def test_fcch_records(rig):
    trk, m, x, fn, F = fcch_case(rig)
    g, rec = rig.slice(trk, m, x, 0, fn, F)
    check_records(g, rec)
    assert [r["ok"] for r in rec[0]] == [True, True] and [r["ok"] for r in rec[1]] == [False, False]
    for r in rec[0]:                                           # placed away from the threshold
        assert abs(r["C"]) ** 2 / r["E"] ** 2 > 0.9
    for r in rec[1]:
        assert r["C"].real <= 0 or abs(r["C"]) ** 2 / r["E"] ** 2 < 0.1
    trk.destroy()


def group_result(pkg, rows, T, n_cols, extra=3):
    """rows: list of (t, c, valid, toa) -> a trxsig_trxgroup_result on the device (and its tensors, to keep them alive)"""
    row = np.full((T, n_cols), -1, np.int32)
    valid, toa = np.zeros(len(rows) + extra, np.uint8), np.zeros(len(rows) + extra, np.float32)
    order = np.random.default_rng(len(rows)).permutation(len(rows) + extra)     # the rows lie anywhere
    for i, (t, c, v, d) in enumerate(rows):
        row[t, c] = order[i]
        valid[order[i]], toa[order[i]] = v, d
    keep = (dev(row), dev(valid), dev(toa))
    res = pkg.TrxGroupResult(n_slots=T, n_arfcn=n_cols, n_rows=len(valid), d_row=keep[0].data_ptr(), d_valid=keep[1].data_ptr(), d_flags=None,
                             d_amp=None, d_toa=keep[2].data_ptr(), d_avgpwr=None, d_threshold=None, d_soft=None, soft_stride=148)
    return res, keep, (row, valid, toa)


def test_update(rig):
    sps, pkg = rig.sps, rig.pkg
    rng = np.random.default_rng(500 + sps)
    q = lambda v: v * sps / 256.0                              # the TOA whose q is v (exact in float32 for small v)
    for with_use in (False, True):
        trk, m, x, fn, F = fcch_case(rig)
        g, rec = rig.slice(trk, m, x, 0, fn, F)
        rel = check_records(g, rec)
        T = 8 * F
        rows = [(0, 0, 1, q(100)), (8, 0, 1, q(100)), (80, 0, 1, q(100)), (88, 0, 1, q(100)),      # C0's TN 0 in frames 0, 1, 10, 11: out
                (16, 0, 1, q(-97)), (1, 0, 1, q(512)), (2, 0, 1, q(-512)), (3, 0, 1, q(513)), (4, 0, 1, q(-513)),   # the gate at equality
                (0, 1, 1, q(-97)), (8, 1, 1, q(-97)), (5, 1, 0, q(400)), (6, 1, 1, np.nan), (7, 1, 1, np.inf), (9, 1, 1, 1e30),
                (0, 2, 1, q(500)), (1, 2, 1, q(-33)), (95, 2, 1, q(-500)), (94, 2, 1, q(1.5 * 256 // sps))]
        rows += [(int(t), 1, 1, q(int(rng.integers(-500, 100)))) for t in rng.choice(np.arange(10, T), 30, replace=False)]
        res, keep, (row, valid, toa) = group_result(pkg, rows, T, 3)
        use = None
        if with_use:
            use = (rng.random((T, 3)) > 0.3).astype(np.uint8)
            use[16, 0], use[8, 1] = 1, 0
            use[:, 2] = 1
        d_use = dev(use) if with_use else None
        step0 = list(m.step)
        trk.update(res, fn, d_use)
        did = m.update(row, valid, toa, fn, use)
        g = trk.collect()
        for p in range(2):
            assert (int(g["toa_sum"][p]), int(g["toa_n"][p]), int(g["adj"][p]), int(g["afc_n"][p])) == (did[p]["S"], did[p]["N"], did[p]["adj"], did[p]["K"]), (p, did[p])
        assert [int(v) for v in g["pos"]] == m.pos and [int(v) for v in g["quiet"]] == m.quiet == [0, 0]
        assert did[0]["K"] == 2 and did[1]["K"] == 0 and did[0]["N"] > 15 and did[1]["N"] == 3 and did[0]["adj"] < 0
        # the phase moved by adj * the step BEFORE the AFC
        assert [int(v) for v in g["phase"]] == m.phase
        # step: acq_atan2's 2e-6 plus the sum's bound, through the shift, plus 1
        bound = int((2.0 ** 32 / (2 * np.pi * sps)) * (2e-6 + rel)) >> 2
        err = [((int(g["step"][p]) - m.step[p] + (1 << 31)) & ltm.M32) - (1 << 31) for p in range(2)]
        print("sps %d: step error %s (bound %d + 1), delta %d" % (sps, err, bound, did[0]["delta"]))
        assert abs(err[0]) <= bound + 1 and err[1] == 0 and m.step[0] != step0[0] and int(g["step"][1]) == step0[1]
        assert abs(int(g["afc_delta"][0]) - did[0]["delta"]) <= (bound << 2) + 4
        # nothing to go by: quiet counts; a second update for the same slice is refused
        assert rig.ctx.L.trxsig_l1trk_update(trk.h, C.byref(res), fn, None) == EINVAL
        m.step[0] = int(g["step"][0])                          # (go on from the device's step: the next slice is compared by words)
        g, rec = rig.slice(trk, m, np.zeros((3, 64), np.complex64), 0, (fn + F) % HYPER, 1)
        res0, keep0, (row0, valid0, toa0) = group_result(pkg, [(3, 0, 0, 0.0)], 8, 3)
        trk.update(res0, (fn + F) % HYPER, None)
        m.update(row0, valid0, toa0, (fn + F) % HYPER)
        g = trk.collect()
        assert list(g["quiet"]) == m.quiet == [1, 1] and [int(v) for v in g["pos"]] == m.pos and list(g["toa_n"]) == [0, 0]
        trk.destroy()


def test_bad_arguments_and_lifetime(rig):
    pkg, ctx, L, sps = rig.pkg, rig.ctx, rig.ctx.L, rig.sps
    before = L.trxsig_live_children(ctx.h)
    trk = pkg.L1Trk(ctx, PHONE, C0, 4)
    assert L.trxsig_live_children(ctx.h) == before + 1
    arr = lambda v: np.ascontiguousarray([0] if v is None else v, np.int32)

    def create(n_phones, n_cols, phone, c0, max_frames=4, afc_shift=1, gate=512, thresh=0.5):
        h = C.c_void_p()
        p, c = arr(phone), arr(c0)
        rc = L.trxsig_l1trk_create(C.byref(h), ctx.h, n_phones, n_cols, p.ctypes.data if phone is not None else None,
                                   c.ctypes.data if c0 is not None else None, max_frames, afc_shift, gate, thresh)
        assert (rc == 0) == bool(h.value)
        if h.value:
            L.trxsig_l1trk_destroy(h)
        return rc
    assert create(2, 3, PHONE, C0) == 0 and create(2, 3, PHONE, [-1, -1]) == 0 and create(3, 3, PHONE, [0, 2, -1]) == 0
    assert create(0, 3, PHONE, C0) == EINVAL and create(2, 0, PHONE, C0) == EINVAL and create(2, 3, None, C0) == EINVAL
    assert create(2, 3, PHONE, None) == EINVAL
    assert create(2, 3, [0, 2, 1], C0) == EINVAL and create(2, 3, [0, -1, 1], C0) == EINVAL        # a column of no phone
    assert create(2, 3, PHONE, [2, 2]) == EINVAL and create(2, 3, PHONE, [0, 3]) == EINVAL and create(2, 3, PHONE, [0, -2]) == EINVAL
    assert create(2, 3, PHONE, C0, max_frames=0) == EINVAL and create(2, 3, PHONE, C0, max_frames=65537) == EINVAL
    assert create(2, 3, PHONE, C0, afc_shift=-1) == EINVAL and create(2, 3, PHONE, C0, afc_shift=9) == EINVAL
    assert create(2, 3, PHONE, C0, afc_shift=0) == 0 and create(2, 3, PHONE, C0, afc_shift=8) == 0
    assert create(2, 3, PHONE, C0, gate=0) == EINVAL and create(2, 3, PHONE, C0, gate=(1 << 24) + 1) == EINVAL
    cell, A, F = 157 * sps, 3, 2
    T = 8 * F
    n = F * 1250 * sps
    d = dev(np.zeros(2 * (A * T * cell + A * n) + 64, np.float32))
    xs, cl = d.data_ptr(), d.data_ptr() + 8 * A * n
    meas = pkg.L1TrkMeas()
    sl = lambda x, ss, ns, fn, F_, c, s1, s2, out=meas: L.trxsig_l1trk_slice(trk.h, x, ss, 0, ns, fn, F_, c, s1, s2, C.byref(out) if out else None)
    assert sl(xs, n, n, 5, F, cl, cell, T * cell) == 0 and meas.n_fcch == 0 and meas.fcch_stride == 1 and meas.n_cols == 3
    assert sl(xs, n, n, 5, F, cl, A * cell, cell) == 0                                            # the other nesting
    assert sl(xs, n, n, 5, 0, cl, cell, T * cell) == EINVAL and sl(xs, n, n, 5, 5, cl, cell, 40 * cell) == EINVAL and sl(xs, n, n, 5, -1, cl, cell, T * cell) == EINVAL
    assert sl(xs, n, n, -1, F, cl, cell, T * cell) == EINVAL and sl(xs, n, n, HYPER, F, cl, cell, T * cell) == EINVAL
    assert sl(xs, n, n, HYPER - 1, F, cl, cell, T * cell) == 0
    assert sl(xs, n, 0, 5, F, cl, cell, T * cell) == EINVAL and sl(xs, n, -4, 5, F, cl, cell, T * cell) == EINVAL
    assert sl(xs, n - 1, n, 5, F, cl, cell, T * cell) == EINVAL                                   # a stride below n_samples
    assert sl(xs, n, n, 5, F, cl, cell - 1, T * cell) == EINVAL and sl(xs, n, n, 5, F, cl, cell, T * cell - 1) == EINVAL
    assert sl(xs, n, n, 5, F, cl, cell, cell) == EINVAL
    assert sl(xs, n, n, 5, F, cl - 8, cell, T * cell) == EINVAL and sl(xs, n, n, 5, F, xs, cell, T * cell) == EINVAL   # cells on the streams
    assert sl(None, n, n, 5, F, cl, cell, T * cell) == EINVAL and sl(xs, n, n, 5, F, None, cell, T * cell) == EINVAL
    assert sl(xs, n, n, 5, F, cl, cell, T * cell, None) == EINVAL
    st = lambda *a: L.trxsig_l1trk_set(trk.h, *a)
    assert st(0, 1, 0, 0, 0, 0) == 0 and st(1, 1, HYPER - 1, -5, 1, 2) == 0
    assert st(2, 1, 0, 0, 0, 0) == EINVAL and st(-1, 1, 0, 0, 0, 0) == EINVAL and st(0, 1, HYPER, 0, 0, 0) == EINVAL and st(0, 1, -1, 0, 0, 0) == EINVAL
    assert L.trxsig_l1trk_state(trk.h, None) == EINVAL
    # update: only the pull of the last slice's cells, once
    res, keep, _ = group_result(pkg, [(1, 0, 1, 0.0)], T, A)
    up = lambda r, fn, u=None: L.trxsig_l1trk_update(trk.h, C.byref(r) if r else None, fn, u)
    assert sl(xs, n, n, 5, F, cl, cell, T * cell) == 0
    assert up(None, 5) == EINVAL and up(res, 6) == EINVAL
    for field, v in (("n_slots", T - 8), ("n_arfcn", A - 1), ("d_row", None), ("d_valid", None), ("d_toa", None)):
        r2, k2, _ = group_result(pkg, [(1, 0, 1, 0.0)], T, A)
        setattr(r2, field, v)
        assert up(r2, 5) == EINVAL, field
    assert up(res, 5) == 0 and up(res, 5) == EINVAL
    # seed: the result of a search, a source per phone
    acq = pkg.L1AcqOut()
    src = dev(arr([-1, -1]))
    assert L.trxsig_l1trk_seed(trk.h, None, src.data_ptr()) == EINVAL and L.trxsig_l1trk_seed(trk.h, C.byref(acq), src.data_ptr()) == EINVAL
    ctx.synchronize()
    assert not d.cpu().numpy()[2 * A * n:].any()              # zero streams in: zeros out, and the refused calls wrote nothing
    trk.destroy()
    assert L.trxsig_live_children(ctx.h) == before


def test_seed(rig):
    """seed from arrays the test lays out as a search's result: state 15 locks with the header's arithmetic, any other state
    unlocks, -1 leaves the phone alone; the negative half, a tie at .5 and an RFN at the hyperframe's end"""
    pkg, sps = rig.pkg, rig.sps
    acq = dict(state=np.array([15, 7, 15, 15], np.uint8), sch_w0=np.array([5000, 1, 0, 123456789], np.int32),
               sch_toa=np.array([12.5, 0, -3.75, 0.49999997], np.float32), omega=np.array([0.03, 0, -0.0314159, 3.1415927], np.float32),
               rfn=np.array([HYPER - 1, 5, 77, 2000000], np.int32))
    keep = {k: dev(v) for k, v in acq.items()}
    out = pkg.L1AcqOut(n_streams=4, soft_stride=148, d_state=keep["state"].data_ptr(), d_sch_w0=keep["sch_w0"].data_ptr(),
                       d_sch_toa=keep["sch_toa"].data_ptr(), d_omega=keep["omega"].data_ptr(), d_rfn=keep["rfn"].data_ptr())
    for src in ([0, 2], [3, 1], [-1, 3], [2, 9]):
        trk, m = rig.pair()
        set_both(trk, m, 0, 1, 9, 99, 999, 9999)
        set_both(trk, m, 1, 1, 8, 88, 888, 8888)
        trk.seed(out, dev(np.array(src, np.int32)))
        m.seed(acq, src)
        same_state(trk.collect(), m)
        trk.destroy()
    assert m.locked == [1, 1] and m.fn == [78, 8]


def test_closed_loop(pkg):
    """The loop of tests/l1_trk_model.py's case on the device (sps 4): see tests/test_l1_trk_model.py for the same loop on the
    model and the reference's detectors, which gave a worst grid error of 0.48 sample and a worst offset error of 1.7e-4
    cycle / symbol."""
    import torch
    import air_loops as al
    import fectxbind
    import l1_msrx_model as lrm
    import test_l1_msrx_model as tm
    tx = fectxbind.FecTxOracle()
    case = ltm.loop_case(tx)
    sps, fn0, F, bsic, band = case["sps"], case["fn0"], case["F"], case["bsic"], case["band"]
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    comb = case["mux"].comb
    A, T = comb.shape[0], 8 * F
    l1 = pkg.L1Tx(ctx, comb, bsic, band)
    l1.set_si(case["mux"].si)
    l1.encode(fn0, F, **{k: dev(v) for k, v in case["grids"].items()})
    enc = l1.collect(state=False)
    assert np.array_equal(enc["what"], case["enc"]["what"]) and np.array_equal(enc["bits"], case["enc"]["bits"])
    sent = np.argwhere(enc["what"] != 0)
    cellw = 157 * sps + 3
    cells = torch.zeros(A * T * cellw, 2, dtype=torch.float32, device="cuda")
    ctx.modulate(dev(enc["bits"][enc["what"] != 0]), dev((8 + (sent[:, 1] % 4 == 0)).astype(np.int32)), cells,
                 dev(((sent[:, 0] * T + sent[:, 1]) * cellw).astype(np.int32)))
    air = pkg.Air(ctx)
    la = ltm.LoopAir(case)

    def stream(r, n0, length, arfcn):
        pr, H = la.params(r, n0), len(arfcn)
        out = torch.zeros(H, length + 5, 2, dtype=torch.float32, device="cuda")
        air.stream(A, T, case["seed"], cells, cellw, T * cellw, out, length + 5, length, dev(np.array(arfcn, np.int32)),
                   dev(np.full(H, pr["cut"], np.int64)), delay=dev(np.full(H, pr["delay"], np.float32)), step=dev_u32(np.full(H, pr["step"])),
                   phase=dev_u32(np.full(H, pr["phase"])), gain=dev_c(np.full(H, case["gain"])), sigma=dev(np.full(H, case["sigma"], np.float32)),
                   n0=dev_u32(np.full(H, pr["n0"])))
        return out
    n = case["n"]
    x = stream(0, 0, n, [0])
    acq = pkg.L1Acq(ctx, 4, n)
    acq.search(x, n + 5, n, 1)
    trk = pkg.L1Trk(ctx, [0, 0], [0], ltm.LOOP_ROUND_FRAMES)
    trk.seed(acq.out, dev(np.array([0], np.int32)))
    g = acq.collect()
    assert int(g["state"][0]) == 15 and int(g["bsic"][0]) == bsic
    st = trk.collect()
    fn_a = int(st["fn"][0])
    span = ltm.LOOP_ROUNDS * ltm.LOOP_ROUND_FRAMES
    assert st["locked"][0] == 1 and fn_a == (int(g["rfn"][0]) + 1) % HYPER and fn0 < fn_a and fn_a + span <= fn0 + F
    e_seed, worst_f = abs(int(st["pos"][0]) - ltm.true_start(case, fn_a, 0)), ltm.step_error(case, 0, int(st["step"][0]))
    print("seed: grid error %.3f sample, offset error %.2e cycle / symbol" % (e_seed, worst_f))
    assert e_seed <= ltm.MAX_SEED and worst_f <= al.MAX_OFFSET
    grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn_a, 0))
    for a in range(A):
        for cmd in ["CMD RXTUNE 935000", "CMD TXTUNE 890000", "CMD SETTSC %d" % (bsic & 7)] + \
                   ["CMD SETSLOT %d %d" % (tn, 3 if tm.PLAN[a, tn] else 0) for tn in range(8)] + ["CMD POWERON"]:
            grp.control(a, cmd)
    rx = pkg.L1MsRx(ctx, comb, bsic, band)
    Fr = ltm.LOOP_ROUND_FRAMES
    Tr, W, lead = 8 * Fr, 160 * sps, 16 * sps
    outs, moves, n_sch, worst_grid = [], 0, 0, 0.0
    for r in range(1, ltm.LOOP_ROUNDS + 1):
        fn_r = int(st["fn"][0])
        n0, ns = ltm.round_plan(case, int(st["pos"][0]), r)
        xs = stream(r, n0, ns, [0, 1])
        buf = torch.zeros(lead + Tr * A * W, 2, dtype=torch.float32, device="cuda")
        base = buf.data_ptr() + 8 * lead
        trk.slice(xs, ns + 5, n0, ns, fn_r, Fr, base, A * W, W)
        res = grp.pull(base, A * W, W, fn_r, 0, Tr)
        grp.sync()
        trk.update(res, fn_r)
        rx.decode(res, fn_r)
        got = rx.collect(state=False)
        outs.append({k: dict(status=got[k + "_status"], frames=got[k], fn=got[k + "_fn"],
                             facch=got["facch"] if k == "tch" else np.zeros(got[k].shape[:2] + (23,), np.uint8),
                             tc=got["bcch_tc"] if k == "bcch" else np.zeros(got[k].shape[:2], np.int32)) for k in ("tch", "xcch", "ccch", "bcch")})
        # every SCH cell through the SCH detector, no shift: a window that starts SCH_LEAD symbols of zeros before the cell
        fs = [f for f in range(Fr) if ((fn_r + f) % HYPER) % 51 in ltm.SCH_T3]
        off = dev(np.array([lead + 8 * f * A * W - ltm.SCH_LEAD * sps for f in fs], np.int32))
        ln = dev(np.full(len(fs), (157 + ltm.SCH_LEAD) * sps, np.int32))
        B = len(fs)
        fl, amp, toa, soft = (torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, 2, device="cuda"), torch.zeros(B, device="cuda"),
                              torch.zeros(B, 148, device="cuda"))
        acq.detect_sch(buf, off, ln, fl, amp, toa, soft)
        ok, bs, rfn = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        ctx.fec_sch_decode(soft, B, ok, bs, rfn)
        st = trk.collect()
        assert (fl.cpu().numpy() & pkg.F_DETECT).all() and ok.cpu().numpy().all() and (bs.cpu().numpy() == bsic).all()
        assert list(rfn.cpu().numpy()) == [(fn_r + f) % HYPER for f in fs]
        n_sch += B
        assert list(st["status"]) == [0, 0] and int(st["fn"][0]) == (fn_r + Fr) % HYPER
        adj, N, K = int(st["adj"][0]), int(st["toa_n"][0]), int(st["afc_n"][0])
        moves += adj != 0
        e, fe = abs(int(st["pos"][0]) - ltm.true_start(case, int(st["fn"][0]), r)), ltm.step_error(case, r, int(st["step"][0]))
        print("round %d: N %d adj %d K %d grid error %.3f sample, offset error %.2e cycle / symbol" % (r, N, adj, K, e, fe))
        assert e <= ltm.MAX_GRID and N > 50 and st["quiet"][0] == 0
        worst_grid = max(worst_grid, e)
        if K:
            assert fe <= al.MAX_OFFSET
            worst_f = max(worst_f, fe)
    print("worst grid error %.3f sample, worst offset error %.2e cycle / symbol, %d moves, %d SCH" % (worst_grid, worst_f, moves, n_sch))
    assert moves >= 1 and n_sch >= 9
    model = lrm.Model(tm.PLAN, bsic, band)
    cnt = ltm.check_span(model, ltm.merge_outputs(outs), case["mux"], case["grids"], case, fn_a, fn_a + span)
    print(cnt)
    assert cnt["tch"] > 20 and cnt["xcch"] > 10 and cnt["ccch"] >= 3 and cnt["bcch"] >= 1, cnt
    trk.destroy(); rx.destroy(); acq.destroy(); air.destroy(); l1.destroy(); grp.close(); ctx.close()
