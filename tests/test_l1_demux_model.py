"""CPU checks of the uplink L1 demultiplexer's model (tests/l1_demux_model.py) and of its recorded mappings
(tests/golden/tdma_uplink.npz): the golden against the reference's GSM/GSMTDMA.cpp where that tree exists, the demux table
against GSM 05.02 facts, the routing under the 5304 / hyperframe wrap."""
import os
import sys

import numpy as np
import pytest

import l1_demux_model as ldm

REF = "/root/reference/GSM/GSMTDMA.cpp"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))


@pytest.fixture(scope="module")
def maps():
    return ldm.load_mappings()


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference tree is not on this machine")
def test_golden_equals_the_reference_tables():
    import gen_tdma_golden
    with open(REF) as f:
        t = gen_tdma_golden.tables(f.read())
    g = np.load(ldm.GOLDEN)
    for k in t:
        assert np.array_equal(t[k], g[k]), k


def test_golden_is_what_gsm_05_02_says(maps):
    assert maps["FACCH_TCHF"].R == 26 and maps["FACCH_TCHF"].frames == [f for f in range(25) if f != 12]
    for tn in range(8):
        m = maps["SACCH_TF_T%d" % tn]
        assert m.R == 104 and m.allowed == 1 << tn
        assert sorted(f % 26 for f in m.frames) == [12 if tn % 2 == 0 else 25] * 4
        assert m.frames == [(m.frames[0] + 26 * i) % 104 for i in range(4)]          # the per-TN rotation
    assert maps["RACHC5"].R == 51 and len(maps["RACHC5"].frames) == 27
    for s in range(8):
        assert maps["SDCCH_8_%dU" % s].frames == [15 + 4 * s + i for i in range(4)]


def plan_table(comb):
    return ldm.install(ldm.plan(np.asarray(comb, np.uint8), ldm.load_mappings(), None), len(comb))


def test_demux_table_facts():
    comb = np.array([[5, 1, 1, 7, 1, 1, 1, 0], [1, 7, 1, 1, 1, 1, 1, 1]], np.uint8)
    t = plan_table(comb)
    for a, tn in ((0, 1), (1, 0), (1, 5)):
        for fn in range(ldm.MAX_MODULUS):
            c = t[a][tn][fn]
            if fn % 26 == 12 or fn % 26 == 25:                # SACCH/TF or idle, never TCH
                assert c is None or c.m.name == "SACCH_TF_T%d" % tn
                assert (c is not None) == (fn % 26 == (12 if tn % 2 == 0 else 25)) or fn % 104 not in c.m.frames
            else:
                assert c.m.name == "FACCH_TCHF"
    rach = {fn % 51 for fn in range(ldm.MAX_MODULUS) if t[0][0][fn] is not None and t[0][0][fn].m.name == "RACHC5"}
    assert rach == {4, 5, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 45, 46}
    used = sum(t[0][0][fn] is not None for fn in range(51))
    assert used == 27 + 16 + 8                                # RACH + 4 SDCCH/4 x 4 + half the SACCH/C4 frames of a 51
    assert t[0][7][0] is None


def test_routing_is_invariant_under_the_wraps():
    comb = np.array([[5, 1, 7, 1, 0, 7, 1, 1]], np.uint8)
    t = plan_table(comb)
    maps = ldm.load_mappings()
    for fn in list(range(0, 300)) + list(range(ldm.HYPERFRAME - 300, ldm.HYPERFRAME)):
        for tn in range(8):
            c = t[0][tn][fn % ldm.MAX_MODULUS]
            c2 = t[0][tn][(fn + ldm.MAX_MODULUS) % ldm.MAX_MODULUS]
            assert c is c2
            if c is not None:
                # B is the same on both sides of the 5304 and of the hyperframe wrap
                n = 8 if c.m.name == "FACCH_TCHF" else 4
                assert c.m.reverse(fn) % n == c.m.reverse(fn + ldm.MAX_MODULUS) % n == \
                    c.m.reverse((fn + ldm.HYPERFRAME) % ldm.HYPERFRAME) % n
    # the B phase of every mapping runs 0, 1, 2, 3 (0..7) in time order across a wrap
    for m in maps.values():
        if m.name == "RACHC5":
            continue
        n = 8 if m.name == "FACCH_TCHF" else 4
        seq = [m.reverse(u % ldm.HYPERFRAME) % n for u in range(ldm.HYPERFRAME - 3 * m.R, ldm.HYPERFRAME + 3 * m.R)
               if m.reverse(u % ldm.HYPERFRAME) >= 0]
        assert all((b - a) % n == 1 for a, b in zip(seq, seq[1:])), m.name


def test_wire_phy():
    assert ldm.wire_phy(37, 0) == (-37, 0)
    assert ldm.wire_phy(200, -255) == (56, 0) and ldm.wire_phy(5, -256) == (-5, -1) and ldm.wire_phy(5, 513) == (-5, 2)
    assert ldm.wire_phy(5, 70000) == (-5, 17)                # 70000 & 0xFFFF = 4464; 4464 / 256 = 17.4


def datagram_phy(rssi, toa):
    """The reference's byte path for one burst's RSSI and timing offset, restated step by step: Transceiver::driveReceiveFIFO
    stores burstString[5] = RSSI (a char: the low byte), burstString[6] = (TOA >> 8) & 0xff, burstString[7] = TOA & 0xff
    (Transceiver.cpp:663-665); ARFCNManager::driveRx reads RSSI = *(signed char *), timingError = (*(signed char *) << 8) |
    next byte, and builds RxBurst(..., timingError / 256.0F, -RSSI) whose int parameter truncates the float (TRXManager.cpp:
    220-233)."""
    b5 = rssi & 0xFF
    b6, b7 = (toa >> 8) & 0xFF, toa & 0xFF
    r = b5 - 256 if b5 >= 128 else b5
    hi = b6 - 256 if b6 >= 128 else b6
    te = (hi << 8) | b7
    q = np.float32(te) / np.float32(256.0)
    return -r, int(q)                                         # C's float -> int conversion: toward zero


def test_wire_narrowing_follows_the_datagram():
    """ldm.wire_phy (what the model applies to collect()'s RSSI / timing) equals the reference's datagram byte path on values
    inside and far outside the signed byte and int16: the boundaries, their wraps, and random values."""
    rng = np.random.default_rng(11)
    rs = list(range(-700, 700)) + [2 ** 31 - 1, -2 ** 31, 255, 256, -255, -256, 383, -385] + rng.integers(-10 ** 6, 10 ** 6, 2000).tolist()
    ts = list(range(-1030, 1030)) + [32767, 32768, 32769, -32768, -32769, -32767, 65535, 65536, 65537, -65536, -65537,
                                     2 ** 31 - 1, -2 ** 31, 98303, -98305] + rng.integers(-4 * 10 ** 7, 4 * 10 ** 7, 4000).tolist()
    for i, t in enumerate(ts):
        r = rs[i % len(rs)]
        assert ldm.wire_phy(r, t) == datagram_phy(r, t), (r, t)
    for r in rs:
        assert ldm.wire_phy(r, 0)[0] == datagram_phy(r, 0)[0], r
    # the signs the wraps produce: 128 dB below full scale reads back as -(-128) = +128, 127 as -127, 32768 / 256 as -128
    assert ldm.wire_phy(128, 0)[0] == 128 and ldm.wire_phy(127, 0)[0] == -127 and ldm.wire_phy(0, 32768)[1] == -128
    assert ldm.wire_phy(0, -255)[1] == 0 and ldm.wire_phy(0, -256)[1] == -1 and ldm.wire_phy(0, 65535)[1] == 0
