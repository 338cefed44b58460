"""The CPU model of the uplink stream decoders (tests/fec_stream_model.py) against the existing batch decoders of the CPU
oracle where the two must agree -- every burst present -- and its FER against an independent float32 recurrence; and the
C-ABI of the stream decoders (exported by libtrxsig.so, declared in include/trxsig.h).  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import fec_stream_model as fsm
import fectxbind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prims():
    return fsm.Prims()


@pytest.fixture(scope="module")
def tx():
    return fectxbind.FecTxOracle()


def fresh(S, tch):
    return np.zeros((S, fsm.TCH_STATE_BYTES if tch else fsm.XCCH_STATE_BYTES), np.uint8)


@pytest.mark.parametrize("wire", [False, True])
def test_xcch_all_present_equals_batch(prims, wire):
    rng = np.random.default_rng(3 + wire)
    S, n = 3, 6
    soft, fr = fsm.xcch_bursts(rng, prims.fo, S, n, noise=0.42)
    soft[1, 8:12] = rng.random((4, 148))                     # one block of noise
    rows = soft.reshape(S * 4 * n, 148)
    index = np.arange(S * 4 * n).reshape(S, 4 * n)
    out = fsm.run(prims, False, rows, index, fresh(S, False), wire=wire)
    seen = set()
    for s in range(S):
        frames, ok = prims.fo.xcch_decode_batch(soft[s], wire=wire)
        assert np.array_equal(out["l2"][s], frames)
        assert np.array_equal(out["status"][s], fsm.DECODED | np.where(ok != 0, fsm.TCH_GOOD, 0))
        seen |= set(ok.tolist())
    assert seen == {0, 1}


@pytest.mark.parametrize("wire", [False, True])
def test_tch_all_present_equals_batch(prims, tx, wire):
    """b0 = 0: slot 7 closes at B = 7, deinterleave(0) over slots 0..7 -- the batch form's block 0.  So stream block m+1
    equals batch block m."""
    rng = np.random.default_rng(5 + wire)
    S, n = 2, 16
    soft, kind, pl = fsm.tch_bursts(rng, tx, S, n, noise=0.4, p_junk=0.12)
    rows = soft.reshape(S * 4 * n, 148)
    index = np.arange(S * 4 * n).reshape(S, 4 * n)
    out = fsm.run(prims, True, rows, index, fresh(S, True), b0=np.zeros(S, np.uint8), wire=wire)
    kinds = set()
    for s in range(S):
        b = prims.fo.tch_decode_batch(soft[s], wire=wire)
        st = out["status"][s, 1:]
        stolen = (st & fsm.STOLEN) != 0
        assert (st & fsm.DECODED).all()
        assert np.array_equal(stolen, b["stolen"] != 0)
        ns = ~stolen
        assert np.array_equal(out["tch"][s, 1:][ns], b["tch"][ns])
        assert np.array_equal((st[ns] & fsm.TCH_GOOD) != 0, b["good"][ns] != 0)
        assert np.array_equal(out["l2"][s, 1:][stolen], b["facch"][stolen])
        assert np.array_equal((st[stolen] & fsm.FACCH_OK) != 0, b["facch_ok"][stolen] != 0)
        assert not out["tch"][s, 1:][stolen].any() and not out["l2"][s, 1:][ns].any()
        kinds |= {(bool(x), bool(y)) for x, y in zip(stolen, (st & (fsm.TCH_GOOD | fsm.FACCH_OK)) != 0)}
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}


def test_fer_is_the_float32_recurrence(prims, tx):
    """d_fer from the model against a recurrence written out here, in float32 with the reference's constants and count
    order, on a stream with missing bursts (a block that is not decoded does not count)."""
    rng = np.random.default_rng(9)
    S, n = 3, 10
    soft, kind, pl = fsm.tch_bursts(rng, tx, S, n, noise=0.45)
    rows = soft.reshape(S * 4 * n, 148)
    index = np.arange(S * 4 * n).reshape(S, 4 * n)
    index[rng.random(index.shape) < 0.2] = -1
    st0 = fresh(S, True)
    st0[:, :4] = np.array([0.3, 0.0, 0.9], np.float32).view(np.uint8).reshape(S, 4)
    out = fsm.run(prims, True, rows, index, st0, b0=np.array([0, 4, 0], np.uint8))
    a = np.float32(1.0) / np.float32(20)
    b = np.float32(1.0) - a
    for s in range(S):
        f = st0[s, :4].view(np.float32)[0]
        for m in range(n):
            flags = int(out["status"][s, m])
            goods = []
            if flags & fsm.DECODED:
                goods = [bool(flags & fsm.FACCH_OK), False] if flags & fsm.STOLEN else [bool(flags & fsm.TCH_GOOD)]
            for g in goods:
                f = np.float32(f * b) if g else np.float32(np.float32(b * f) + a)
            assert out["fer"][s, m].view(np.uint32) == np.float32(f).view(np.uint32), (s, m)
        assert out["state"][s, :4].view(np.float32)[0] == f
    assert (out["status"] & fsm.DECODED).any() and not (out["status"] & fsm.DECODED).all()


def test_model_missing_bursts_and_fresh_rows(prims, tx):
    """A fresh decoder's rows are 0.0: block 0 (closing at B = 3) reads rows 4..7 as zeros; a consumed position reads 0.5
    later; a block whose closing burst is missing is not decoded and its rows stay for the next block."""
    rng = np.random.default_rng(11)
    soft, _, _ = fsm.tch_bursts(rng, tx, 1, 4)
    rows = soft.reshape(16, 148)
    d = fsm.Decoder(prims, True)
    for t in range(4):
        d.burst(t, prims.wire(rows[t]))
    # rows 4..7 never written: their even halves were read as 0.0 and consumed (0.5), the odd halves are still 0.0
    assert (d.mI[4:, 0::2] == np.float32(0.5)).all() and (d.mI[4:, 1::2] == 0).all()
    assert (d.mI[:4, 1::2] == np.float32(0.5)).all()
    # stream: slot 7 (a closing slot) missing -> block 1 is not decoded, block 2 reads the stale rows
    index = np.arange(16)[None].copy()
    index[0, 7] = -1
    out = fsm.run(prims, True, rows, index, fresh(1, True), b0=np.zeros(1, np.uint8))
    assert out["status"][0, 1] == 0 and out["status"][0, 2] & fsm.DECODED
    assert out["fer"][0, 1] == out["fer"][0, 0]


def test_chaining_in_the_model(prims, tx):
    rng = np.random.default_rng(13)
    S, n = 2, 8
    soft, _, _ = fsm.tch_bursts(rng, tx, S, n)
    rows = soft.reshape(S * 4 * n, 148)
    index = np.arange(S * 4 * n).reshape(S, 4 * n)
    index[rng.random(index.shape) < 0.25] = -1
    b0 = np.array([0, 4], np.uint8)
    whole = fsm.run(prims, True, rows, index, fresh(S, True), b0=b0)
    st = fresh(S, True)
    for lo, hi in ((0, 12), (12, 16), (16, 32)):
        part = fsm.run(prims, True, rows, index[:, lo:hi], st, b0=(b0 + lo) % 8)
        for k in ("status", "tch", "l2", "fer"):
            assert np.array_equal(part[k], whole[k][:, lo // 4:hi // 4])
        st = part["state"]
    assert np.array_equal(st, whole["state"])


def test_stream_decoders_in_the_abi():
    """The stream decoders are exported by libtrxsig.so and declared in include/trxsig.h with their state sizes."""
    so = os.path.join(ROOT, "openbts-ttsou_amd", "libtrxsig.so")
    lib = ctypes.CDLL(so)
    for name in ("trxsig_fec_tch_decode_stream", "trxsig_fec_xcch_decode_stream"):
        assert hasattr(lib, name), name
    h = open(os.path.join(ROOT, "include", "trxsig.h")).read()
    assert re.search(r"int trxsig_fec_tch_decode_stream\(trxsig_ctx \*ctx, int n_chan, int n_slots, const float \*d_soft", h)
    assert re.search(r"int trxsig_fec_xcch_decode_stream\(trxsig_ctx \*ctx, int n_chan, int n_slots, const float \*d_soft", h)
    assert "#define TRXSIG_TCH_RX_STATE_BYTES %d" % fsm.TCH_STATE_BYTES in h
    assert "#define TRXSIG_XCCH_RX_STATE_BYTES %d" % fsm.XCCH_STATE_BYTES in h
    for k, v in (("DECODED", 1), ("STOLEN", 2), ("FACCH_OK", 4), ("TCH_GOOD", 8)):
        assert re.search(r"TRXSIG_FEC_%s = %d\b" % (k, v), h)
    assert "TRXSIG_K_COUNT = 15" in h
