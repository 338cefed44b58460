"""The downlink L1 multiplexer's CPU model (tests/l1_mux_model.py) against what it restates: the golden against GSMTDMA.cpp,
combination V's beacon frames, encodePower, the SACCH order arithmetic, the SACCH header at bit level and split-call
invariance in the model itself."""
import os

import numpy as np
import pytest

import l1_mux_model as lmm

REF = os.environ.get("OPENBTS_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def oracle():
    import fectxbind
    return fectxbind.FecTxOracle()


def test_golden_equals_the_reference_tables():
    path = os.path.join(REF, "GSM", "GSMTDMA.cpp")
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gdl", os.path.join(os.path.dirname(__file__), "..", "tools",
                                                                      "gen_tdma_downlink_golden.py"))
    gdl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gdl)
    with open(path) as f:
        t = gdl.tables(f.read())
    g = np.load(lmm.GOLDEN)
    for k in t:
        assert np.array_equal(np.asarray(t[k]), g[k]), k


def test_combination_v_carries_each_channel_on_its_frames():
    """Over 102 frames, C0 T0 under combination V carries FCCH, SCH, BCCH, CCCH_0-2, SDCCH/4 and SACCH/C4 exactly on their
    GSM 05.02 frames, and no two channels of any plan share a (TN, FN)."""
    maps = lmm.load_mappings()
    expect = {"FCCH": [0, 10, 20, 30, 40], "SCH": [1, 11, 21, 31, 41], "BCCH": [2, 3, 4, 5], "CCCH_0": [6, 7, 8, 9],
              "CCCH_1": [12, 13, 14, 15], "CCCH_2": [16, 17, 18, 19], "SDCCH_4_0D": [22, 23, 24, 25],
              "SDCCH_4_1D": [26, 27, 28, 29], "SDCCH_4_2D": [32, 33, 34, 35], "SDCCH_4_3D": [36, 37, 38, 39]}
    owner = {}
    for name, fr in expect.items():
        got = [k for k, _ in lmm.MuxModel.walk(maps[name], 0, 102)]
        assert got == fr + [f + 51 for f in fr], name
    sacch = {"SACCH_C4_0D": [42, 43, 44, 45], "SACCH_C4_1D": [46, 47, 48, 49], "SACCH_C4_2D": [93, 94, 95, 96],
             "SACCH_C4_3D": [97, 98, 99, 100]}
    for name, fr in sacch.items():
        assert [k for k, _ in lmm.MuxModel.walk(maps[name], 0, 102)] == fr, name
    for combo in (["FCCH", "SCH", "BCCH", "CCCH_0", "CCCH_1", "CCCH_2"] + ["SDCCH_4_%dD" % s for s in range(4)] +
                  ["SACCH_C4_%dD" % s for s in range(4)],
                  ["SDCCH_8_%dD" % s for s in range(8)] + ["SACCH_C8_%dD" % s for s in range(8)]):
        owner = {}
        for name in combo:
            for k, _ in lmm.MuxModel.walk(maps[name], 0, 204):
                assert k not in owner, (name, owner.get(k), k)
                owner[k] = name
    for tn in range(8):
        owner = {}
        for name in ("FACCH_TCHF", "SACCH_TF_T%d" % tn):
            for k, _ in lmm.MuxModel.walk(maps[name], 0, 208):
                assert k not in owner, (name, k)
                owner[k] = name
        assert len(owner) == 208 - 8                             # one idle frame per 26


@pytest.mark.parametrize("band", [900, 1800, 1900])
def test_encode_power(band):
    t = lmm.POWER[band]
    for code, dbm in enumerate(t):
        assert t[lmm.encode_power(band, dbm)] == dbm          # exact values: the first code from 1 on that has it (the loop
        assert lmm.encode_power(band, dbm) == next((i for i in range(1, 32) if t[i] == dbm), 0)   # returns there), else 0
    assert lmm.encode_power(band, 100) == t.index(max(t))      # out of the table: nearest
    assert lmm.encode_power(band, -100) == t.index(min(t))
    if band == 900:
        assert lmm.encode_power(band, 38) == 0 and lmm.encode_power(band, 36) == 3   # ties: the first code
    else:
        assert lmm.encode_power(band, 29) == 0 and lmm.encode_power(band, 27) == 1


def test_order_arithmetic_clamps_and_halfway_cases():
    # deltaP * 0.5 = +-x.5 rounds away from zero (C's round), not to even
    assert lmm.sacch_orders(-10, -15.0, 30, 0, 0)[0] == 30 - 3      # 5 * 0.5 = 2.5 -> 3
    assert lmm.sacch_orders(-20, -15.0, 30, 0, 0)[0] == 30 + 3      # -2.5 -> -3
    assert lmm.sacch_orders(-14, -15.0, 30, 0, 0)[0] == 30 - 1      # 0.5 -> 1
    assert lmm.sacch_orders(100, -15.0, 30, 0, 0)[0] == 0
    assert lmm.sacch_orders(-120, -15.0, 30, 0, 0)[0] == 40
    assert lmm.sacch_orders(-15, -15.0, 40, 0, 0)[0] == 40
    assert lmm.sacch_orders(-15, -15.0, 0, 0, 0)[0] == 0
    assert lmm.sacch_orders(0, -15.0, 0, 63, -10)[1] == np.float32(63.0)
    assert lmm.sacch_orders(0, -15.0, 0, 0, 10)[1] == np.float32(0.0)
    assert lmm.sacch_orders(0, -15.0, 0, 10, 3)[1] == np.float32(8.5)
    assert lmm.sacch_header(900, 30, np.float32(8.5)) == (lmm.encode_power(900, 30), 9)
    assert lmm.sacch_header(900, 30, np.float32(8.49)) == (lmm.encode_power(900, 30), 8)
    assert lmm.c_round(2.5) == 3 and lmm.c_round(-2.5) == -3 and round(2.5) == 2


def test_sacch_block_bit_level(oracle):
    """A SACCH block in the model equals the restatement: mU.fillField of the header, the frame copied in at bit 16, LSB8MSB,
    Fire parity, the coder and the 4.1.4 interleave."""
    rng = np.random.default_rng(3)
    comb = np.array([[5, 1, 0, 0, 0, 0, 0, 0]], np.uint8)
    model = lmm.MuxModel(comb, 12, oracle=oracle)
    for trial in range(6):
        power, ta = int(rng.integers(0, 41)), np.float32(rng.integers(0, 127) / 2)
        l2 = rng.integers(0, 256, 23).astype(np.uint8)
        got = oracle.xcch_encode(model.sacch_frame(l2, power, ta), model.tsc)
        u = np.zeros(228, np.uint8)
        code, tav = lmm.encode_power(900, power), int(np.float32(ta + np.float32(0.5)))
        u[0:8] = [(code >> (7 - i)) & 1 for i in range(8)]                       # fillField(0, code, 8)
        u[8:16] = [(tav >> (7 - i)) & 1 for i in range(8)]                       # fillField(8, ta, 8)
        u[16:184] = np.unpackbits(l2[2:])                                        # frame.copyToSegment(mU, 16)
        u[:184] = oracle.lsb8msb(u[:184])
        pw = ~oracle.parity(0x10004820009, 40, u[:184]) & ((1 << 40) - 1)
        u[184:224] = [(pw >> (39 - k)) & 1 for k in range(40)]
        c = oracle.encode(u)
        want = np.zeros((4, 148), np.uint8)
        want[:, 60] = want[:, 87] = 1
        want[:, 61:87] = model.tsc
        for k in range(456):
            B, j = k % 4, 2 * ((49 * k) % 57) + ((k % 8) // 4)
            want[B, 3 + j if j < 57 else 88 + j - 57] = c[k]
        assert np.array_equal(got, want), trial


def test_split_calls_in_the_model(oracle):
    rng = np.random.default_rng(9)
    comb = np.array([[5, 1, 7, 1, 0, 0, 0, 0]], np.uint8)
    si = rng.integers(0, 256, (4, 23)).astype(np.uint8)
    content = {}

    def grids(model, fn, F):
        out = []
        nb = model.grid(fn, F)
        for cls, w, n in ((lmm.TCH, 33, nb[0]), (lmm.XCCH, 23, nb[1]), (lmm.CCCH, 23, nb[2])):
            ch = model.ch[cls]
            kind = np.zeros((len(ch), n), np.uint8); pay = np.zeros((len(ch), n, w), np.uint8)
            for i, c in enumerate(ch):
                b = 0
                for k, B in model.walk(c.m, fn, F):
                    if B == 0:
                        key = (cls, i, fn + k)
                        if key not in content:
                            content[key] = (int(rng.integers(0, 3)) if cls == lmm.TCH else int(rng.integers(0, 2)),
                                            rng.integers(0, 256, w).astype(np.uint8))
                        kind[i, b], pay[i, b] = content[key]
                        b += 1
            out += [kind, pay]
        return out

    fn0, F = 5304 * 3 - 40, 120
    whole = lmm.MuxModel(comb, 7, oracle=oracle); whole.set_si(si)
    split = lmm.MuxModel(comb, 7, oracle=oracle); split.set_si(si)
    w = whole.encode(fn0, F, *grids(whole, fn0, F))
    edges = [0, 1, 3, 30, 31, 77, F]
    parts = [split.encode(fn0 + lo, hi - lo, *grids(split, fn0 + lo, hi - lo)) for lo, hi in zip(edges[:-1], edges[1:])]
    assert np.array_equal(np.concatenate([p["bits"] for p in parts], 1), w["bits"])
    assert np.array_equal(np.concatenate([p["what"] for p in parts], 1), w["what"])
    assert (w["what"] == lmm.W_TCH).any() and (w["what"] == lmm.W_BCCH).any() and (w["what"] == lmm.W_SCH).any()
