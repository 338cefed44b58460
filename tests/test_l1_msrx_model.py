"""The CPU model of the mobile-side downlink L1 (tests/l1_msrx_model.py) on its own -- no GPU.  The downlink mappings share no
frame on any slot of combinations I, V and VII; what tests/l1_mux_model.py (the downlink multiplexer's literal model) encodes
comes back as its payloads; SCH bursts of the compiled downlink-encode oracle decode to their FN and BSIC; one call equals any
split of it."""
import numpy as np
import pytest

import fec_stream_model as fsm
import fectxbind
import l1_msrx_model as lrm
import l1_mux_model as lmm

HYPER = lrm.HYPERFRAME


@pytest.fixture(scope="module")
def prims():
    return fsm.Prims()


@pytest.fixture(scope="module")
def tx():
    return fectxbind.FecTxOracle()


def test_downlink_mappings_are_disjoint_on_every_slot():
    maps = lrm.load_mappings()
    for comb, owned in ((1, 25 * 4), (5, 100), (7, 2 * 32 + 32)):   # frames owned per 104 (I) / 102 (V, VII): the rest is idle
        for tn in range(8):
            table, clash = lrm.slot_table(maps, comb, tn)
            assert not clash, (comb, tn, clash[:3])
            period = 104 if comb == 1 else 102
            assert sum(x is not None for x in table) == owned * (lrm.MAX_MODULUS // period), (comb, tn)
    table, _ = lrm.slot_table(maps, 5, 0)
    assert [table[f] for f in (0, 1, 2, 6, 10, 11, 50)] == ["FCCH", "SCH", "BCCH", "CCCH_0", "FCCH", "SCH", None]


def fn_of(t1, t2, t3):
    return 1326 * t1 + 51 * ((t3 - t2) % 26) + t3


def test_sch_decoder_inverts_the_encode_oracle(tx):
    cases = [(t1, t2, t3, bsic) for t1 in (0, 1, 2047) for t2 in range(26) for t3 in (1, 11, 21, 31, 41) for bsic in (0, 21, 63)]
    fns = np.array([fn_of(t1, t2, t3) for t1, t2, t3, _ in cases], np.uint32)
    assert all(int(f) % 26 == c[1] and int(f) % 51 == c[2] and int(f) // 1326 == c[0] for f, c in zip(fns, cases))
    bits = tx.sch_encode(fns, np.array([c[3] for c in cases], np.uint8))
    rng = np.random.default_rng(1)
    for v, f, c in zip(fsm.soft_from_bits(rng, bits, 0.3), fns, cases):
        assert lrm.sch_decode(tx, tx.wire(v)) == (True, c[3], int(f)), c
    flipped = bits[7].copy()
    flipped[[3 + 2 * i for i in range(10)] + [106 + 3 * i for i in range(10)]] ^= 1
    assert not lrm.sch_decode(tx, flipped.astype(np.float32))[0]


PLAN = np.array([[5, 1, 7, 0, 1, 0, 0, 0], [1, 7, 0, 0, 0, 0, 0, 1]], np.uint8)


def random_grids(rng, mux, fn, F):
    """random payloads for every block of a call of the multiplexer (or of its model): speech / FACCH on TCH, L2 frames elsewhere"""
    nbt, nbx, nbc = mux.grid(fn, F)
    g = dict(tch_kind=rng.choice(np.array([1, 1, 2], np.uint8), (len(mux.ch[lmm.TCH]), nbt)),
             tch_payload=rng.integers(0, 256, (len(mux.ch[lmm.TCH]), nbt, 33)).astype(np.uint8),
             xcch_kind=np.ones((len(mux.ch[lmm.XCCH]), nbx), np.uint8),
             xcch_payload=rng.integers(0, 256, (len(mux.ch[lmm.XCCH]), nbx, 23)).astype(np.uint8),
             ccch_kind=np.ones((len(mux.ch[lmm.CCCH]), nbc), np.uint8),
             ccch_payload=rng.integers(0, 256, (len(mux.ch[lmm.CCCH]), nbc, 23)).astype(np.uint8))
    g["tch_payload"][:, :, 32] &= 0xF0
    return g


def encode_cell(rng, tx, fn, F, bsic=21, band=900, comb=PLAN):
    """tests/l1_mux_model.py over a plan: random payloads on every channel, SIs set.  Returns (mux model, its output, the grids)."""
    mux = lmm.MuxModel(comb, bsic, band=band, oracle=tx)
    mux.set_si(rng.integers(0, 256, (4, 23)).astype(np.uint8))
    g = random_grids(rng, mux, fn, F)
    return mux, mux.encode(fn, F, **g), g


def sent_blocks(mux, fn, F):
    """(class, channel, block b) -> the unwrapped frame of the block's first burst, for every block the call opens"""
    out = {}
    for cls in (lmm.TCH, lmm.XCCH, lmm.CCCH, lmm.BCCH):
        for i, c in enumerate(mux.ch[cls]):
            for b, k in enumerate(k for k, B in mux.walk(c.m, fn, F) if B == 0):
                out[(cls, i, b)] = fn + k
    return out


def check_payloads(model, out, mux, grids, fn, F, si, band, skip=()):
    """every block the multiplexer sent whole inside [fn, fn + F) is in `out` with its payload; skip: (class, channel) pairs of
    the multiplexer's that sent nothing (closed)"""
    n = dict(tch=0, xcch=0, ccch=0, bcch=0)
    for (cls, i, b), first in sent_blocks(mux, fn, F).items():
        if (cls, i) in skip:
            continue
        key = lrm.KEYS[{lmm.TCH: lrm.TCH, lmm.XCCH: lrm.XCCH, lmm.CCCH: lrm.CCCH, lmm.BCCH: lrm.BCCH}[cls]]
        c = model.ch[{"tch": lrm.TCH, "xcch": lrm.XCCH, "ccch": lrm.CCCH, "bcch": lrm.BCCH}[key]][i]
        o = out[key]
        if cls == lmm.TCH:                                   # a TCH block's second half rides the next block's bursts
            closing = model.next_closing(c, model.next_closing(c, first) + 1)
        else:
            closing = model.next_closing(c, first)
        if closing >= fn + F:
            continue
        col = list(o["fn"][i]).index(closing % HYPER)
        st = int(o["status"][i, col])
        if cls == lmm.TCH:
            if grids["tch_kind"][i, b] == 1:
                assert st == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(o["frames"][i, col], grids["tch_payload"][i, b]), (i, b)
            else:
                assert st & fsm.FACCH_OK and np.array_equal(o["facch"][i, col], grids["tch_payload"][i, b, :23]), (i, b)
        else:
            assert st == fsm.DECODED | fsm.TCH_GOOD, (key, i, b, st)
            fr = o["frames"][i, col]
            if cls == lmm.BCCH:
                tc = ((first % HYPER) // 51) % 8
                assert o["tc"][i, col] == tc and np.array_equal(fr, si[lmm.SI_OF_TC[tc]]), (i, b)
            else:
                want = grids["xcch_payload" if cls == lmm.XCCH else "ccch_payload"][i, b]
                assert np.array_equal(fr[2:], want[2:]), (key, i, b)
                if not c.sacch:
                    assert np.array_equal(fr[:2], want[:2])
        n[key] += 1
    return n


def test_what_the_multiplexer_model_encodes_comes_back(prims, tx):
    rng = np.random.default_rng(11)
    fn, F = 5304 * 2 + 17, 208
    mux, enc, grids = encode_cell(rng, tx, fn, F)
    model = lrm.Model(PLAN, 21, prims=prims)
    out = model.decode(lrm.col_from_bits(rng, enc["bits"], enc["what"], 0.3), fn)
    n = check_payloads(model, out, mux, grids, fn, F, mux.si, 900)
    assert n["tch"] > 20 and n["xcch"] > 40 and n["ccch"] >= 9 and n["bcch"] >= 3, n
    s, f = out["sch"], out["fcch"]
    assert len(s["fn"]) >= 20 and len(f["fn"]) >= 20 and s["sync"].all() and (s["rfn"] == s["fn"]).all() and (s["bsic"] == 21).all()
    assert (f["ones"] == 0).all()
    # the SACCH header of a multiplexer without a sibling: 40 dBm to the band's nearest level, TA 0
    x = out["xcch"]
    sacch = np.array([c.sacch for c in model.ch[lrm.XCCH]])
    assert (x["power"][sacch] == 39).all() and (x["ta"][sacch] == 0).all() and (x["power"][~sacch] == -1).all()


def test_one_call_equals_any_split(prims, tx):
    rng = np.random.default_rng(12)
    fn, F = HYPER - 70, 160
    mux, enc, _ = encode_cell(rng, tx, fn, F)
    col = lrm.col_from_bits(rng, enc["bits"], None, 0.3)
    col["valid"] &= rng.random(col["valid"].shape) > 0.1
    col["rssi"] = rng.integers(-300, 300, col["valid"].shape)
    col["timing"] = rng.integers(-40000, 40000, col["valid"].shape)
    whole = lrm.Model(PLAN, 21, prims=prims)
    whole.ch[lrm.XCCH][3].active = False
    ow = whole.decode(col, fn)
    part = lrm.Model(PLAN, 21, prims=prims)
    part.ch[lrm.XCCH][3].active = False
    cuts = [0] + sorted(rng.choice(np.arange(1, F), 5, replace=False).tolist()) + [F]
    blocks, lists = {}, []
    for lo, hi in zip(cuts, cuts[1:]):
        o = part.decode(lrm.cut(col, lo, hi), (fn + lo) % HYPER)
        blocks.update(lrm.blocks_by_fn(o))
        lists.append(o)
    assert blocks == lrm.blocks_by_fn(ow) and len(blocks) > 100
    for key in ("tch", "xcch", "ccch", "bcch"):
        for k in ("state", "rssi", "timing"):
            assert np.array_equal(o[key][k], ow[key][k]), (key, k)
    assert np.array_equal(o["xcch"]["power"], ow["xcch"]["power"]) and np.array_equal(o["xcch"]["ta"], ow["xcch"]["ta"])
    for key in ("sch", "fcch"):
        for k in ow[key]:
            assert np.array_equal(np.concatenate([x[key][k] for x in lists]), ow[key][k]), (key, k)
    assert not ow["sch"]["present"].all() and ow["sch"]["sync"].any() and (ow["fcch"]["ones"] == -1).any()
