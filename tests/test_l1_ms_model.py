"""The literal model of the mobile-side uplink L1 (tests/l1_ms_model.py) against the uplink demultiplexer's model
(tests/l1_demux_model.py) and the decode oracle: what it sends comes back.  No GPU."""
import numpy as np
import pytest

import fec_stream_model as fsm
import l1_demux_model as ldm
import l1_ms_model as lms

HYPER = lms.HYPERFRAME


@pytest.fixture(scope="module")
def oracle():
    import fectxbind
    return fectxbind.FecTxOracle()


@pytest.fixture(scope="module")
def prims():
    return fsm.Prims()


def mixed_plan():
    comb = np.zeros((2, 8), np.uint8)
    comb[0, :3] = [5, 1, 7]; comb[0, 4] = 1; comb[1, :2] = [1, 7]
    return comb


def blocks(model, c, fn, F):
    """The channel's blocks of a call: (first frame, closing frame or None where it lies past the call), unwrapped"""
    w = model.walk(c.m, fn, F)
    out = []
    for j, (k, B) in enumerate(w):
        if B == 0:
            out.append((fn + k, fn + w[j + 3][0] if j + 3 < len(w) else None))
    return out


def test_everything_sent_comes_back(oracle, prims):
    """A = 2, F = 208, every combination: the model's bursts as 0 / 1 soft values through l1_demux_model.Model return every
    speech, FACCH, SDCCH and SACCH payload, every RA sent with the cell's BSIC (the others refused), and the handsets' power / TA."""
    rng = np.random.default_rng(41)
    comb, bsic, band, fn0, F = mixed_plan(), 21, 1800, 26 * 40, 208
    ms = lms.MsModel(comb, bsic, band, oracle=oracle)
    rx = ldm.Model(comb, bsic, band=band, prims=prims)
    sacch = [i for i, c in enumerate(ms.ch[lms.XCCH]) if c.sacch]
    for i in sacch[::2]:
        ms.set_phy(i, int(rng.integers(0, 41)), int(rng.integers(0, 64)))
    content = lms.Content(rng, p_none=0.1, speech=True)
    g = lms.grids(ms, content, fn0, F)
    m = ms.encode(fn0, F, **g)
    T = 8 * F
    col = dict(valid=(m["what"] != 0).T, soft=m["bits"].transpose(1, 0, 2).astype(np.float32), rssi=np.zeros((T, 2), np.int64),
               timing=np.zeros((T, 2), np.int64))
    d = rx.decode(col, fn0)
    # TCH: the decoder's block b carries the encoder's block b - 1 (fn0 is on the 26-frame grid)
    n_speech = n_facch = 0
    for s in range(len(ms.ch[lms.TCH])):
        for b in range(1, g["tch_kind"].shape[1]):
            kind, pl = g["tch_kind"][s, b - 1], g["tch_payload"][s, b - 1]
            if kind == 1:
                assert d["tch"]["status"][s, b] == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(d["tch"]["frames"][s, b], pl), (s, b)
                n_speech += 1
            else:
                assert d["tch"]["status"][s, b] & fsm.FACCH_OK and np.array_equal(d["tch"]["facch"][s, b], pl[:23]), (s, b)
                n_facch += 1
    assert n_speech > 60 and n_facch > 20                    # 3 channels x 47 blocks, 70 % speech
    # XCCH: every block sent whole inside the call decodes to its frame, SACCH frames with the handset's header
    n_sd = n_sa = 0
    heard = []                                               # SACCH channels the decoder got a whole frame of
    for s, c in enumerate(ms.ch[lms.XCCH]):
        for b, (first, closing) in enumerate(blocks(ms, c, fn0, F)):
            if closing is None or g["xcch_kind"][s, b] != 1:
                continue
            want = g["xcch_payload"][s, b].copy()
            if c.sacch:
                want[0], want[1] = lms.lmm.encode_power(band, c.power) & 31, c.ta
                n_sa += 1
                heard.append(s)
            else:
                n_sd += 1
            j = list(d["xcch"]["fn"][s]).index(closing % HYPER)
            assert d["xcch"]["status"][s, j] == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(d["xcch"]["frames"][s, j], want), (s, b)
    assert n_sd > 30 and n_sa > 8
    heard = sorted(set(heard))                               # (a decoder that heard nothing keeps its own 40 dBm / 0)
    assert len(heard) >= len(sacch) - 2
    assert np.array_equal(d["xcch"]["power"][heard], m["ms_power"][heard]) and np.array_equal(d["xcch"]["ta"][heard], m["ms_ta"][heard])
    assert (m["ms_power"] == -1).sum() == len(ms.ch[lms.XCCH]) - len(sacch)
    assert len({(p, t) for p, t in zip(m["ms_power"][sacch], m["ms_ta"][sacch])}) > 3
    # RACH: every access burst is listed in FN order; RA back where the BSIC is the cell's
    sent = [(fn0 + k, g["rach_ra"][j], g["rach_bsic"][j]) for j, (k, _) in enumerate(ms.walk(ms.ch[lms.RACH][0].m, fn0, F))
            if g["rach_kind"][j] == 1]
    r = d["rach"]
    assert list(r["fn"]) == [u % HYPER for u, _, _ in sent] and len(sent) > 50
    for (u, ra, b), ok, got in zip(sent, r["ok"], r["ra"]):
        assert ok == (b == bsic) and got == (ra if b == bsic else 0), u
    assert r["ok"].any() and not r["ok"].all()


def test_every_access_burst_decodes(oracle):
    """All 256 RA x 64 BSIC through the oracle's rach_decode."""
    for bsic in range(64):
        for ra in range(256):
            r = oracle.rach_decode(lms.rach_e36(oracle, ra, bsic).astype(np.float32))
            assert r["tail_ok"] and int(r["bsic"]) == bsic and int(r["ra"]) == ra, (ra, bsic)
    b = lms.access_burst(oracle, 0xA5, 7)
    assert list(b[:8]) == [0, 0, 1, 1, 1, 0, 1, 0] and not b[85:].any()


@pytest.mark.parametrize("fn0", [26 * 51 * 3 - 50, HYPER - 61])
def test_split_calls_equal_one_call(oracle, fn0):
    rng = np.random.default_rng(fn0 % 991)
    comb, F = mixed_plan(), 130
    content = lms.Content(rng)
    whole, parts = lms.MsModel(comb, 9, oracle=oracle), lms.MsModel(comb, 9, oracle=oracle)
    for m in (whole, parts):
        m.set_phy(4, 17, 33)
        m.close(lms.XCCH, 2)
    w = whole.encode(fn0, F, **lms.grids(whole, content, fn0, F))
    cuts = [0, 1, 2, 37, 61, 62, 90, F]
    out = [parts.encode(fn0 + lo, hi - lo, **lms.grids(parts, content, fn0 + lo, hi - lo)) for lo, hi in zip(cuts, cuts[1:])]
    for k in ("bits", "what"):
        assert np.array_equal(np.concatenate([o[k] for o in out], axis=1), w[k]), k
    for k in ("tch_state", "xcch_state", "ms_power", "ms_ta"):
        assert np.array_equal(out[-1][k], w[k]), k
    assert {lms.W_TCH, lms.W_XCCH, lms.W_ACCESS} <= set(np.unique(w["what"]).tolist())
