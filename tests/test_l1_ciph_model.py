"""The model of the ciphering stage (tests/l1_ciph_model.py) against the published A5/1 vector, its own word-for-word form, and
the encoders' models: what it routes is what they write.  No GPU."""
import numpy as np
import pytest

import l1_ciph_model as lcm
import l1_ms_model as lms
import l1_mux_model as lmm

HYPER = lcm.HYPERFRAME
KC = bytes.fromhex("1223456789ABCDEF")
BLOCK1 = bytes.fromhex("534EAA582FE8151AB6E1855A728C00")
BLOCK2 = bytes.fromhex("24FD35A35D5FB6526D32F906DF1AC0")


def small_plan():
    comb = np.zeros((2, 8), np.uint8)
    comb[0, :3] = [5, 7, 1]; comb[1, 0] = 1
    return comb


def test_published_vector():
    b1, b2 = lcm.a5_1(KC, 0x134)
    assert b1.shape == b2.shape == (114,)
    assert np.packbits(b1).tobytes() == BLOCK1 and np.packbits(b2).tobytes() == BLOCK2
    v1, v2 = lcm.blocks_batch([list(KC)], [0x134])          # the array form the operations use
    assert np.array_equal(v1[0], b1) and np.array_equal(v2[0], b2)


def test_array_form_equals_the_statement():
    rng = np.random.default_rng(3)
    kc = rng.integers(0, 256, (9, 8)).astype(np.uint8)
    count = rng.integers(0, 1 << 22, 9).astype(np.uint32)
    v1, v2 = lcm.blocks_batch(kc, count)
    for i in range(9):
        b1, b2 = lcm.a5_1(kc[i], int(count[i]))
        assert np.array_equal(v1[i], b1) and np.array_equal(v2[i], b2), i
    assert len({v.tobytes() for v in v1}) == 9


def test_zero_is_a_fixed_point():
    b1, b2 = lcm.a5_1(bytes(8), 0)
    assert not b1.any() and not b2.any() and lcm.key_registers(bytes(8)) == (0, 0, 0)
    b1, _ = lcm.a5_1(bytes(8), 1)                           # the count alone moves the registers
    assert b1.any()


def test_count():
    assert int(lcm.count_of(0)) == 0
    assert int(lcm.count_of(1325)) == (1325 % 51) << 5 | 1325 % 26 == (50 << 5) | 25
    assert int(lcm.count_of(1326)) == 1 << 11
    assert int(lcm.count_of(HYPER - 1)) == (2047 << 11) | (50 << 5) | 25 == 0x3FFE59
    assert list(lcm.count_of([0, 51, 26])) == [0, 25, 26 << 5]


def test_directions_differ_and_the_operation_is_an_involution():
    rng = np.random.default_rng(5)
    comb = small_plan()
    m = lcm.CiphModel(comb)
    for cls in (lcm.TCH, lcm.XCCH):
        for i in range(len(m.ch[cls])):
            m.set(cls, i, lcm.A5_1, rng.integers(0, 256, 8).astype(np.uint8))
    fn, F = 1326 * 3 - 20, 60
    bits = rng.integers(0, 2, (2, 8 * F, 148)).astype(np.uint8)
    on_d, ks_d = m.slot_keystream(0, fn, F)
    on_u, ks_u = m.slot_keystream(1, fn, F)
    both = on_d & on_u
    assert both.sum() > 100 and (ks_d[both] != ks_u[both]).any(axis=-1).all()      # BLOCK2 of FN is not BLOCK1 of FN
    for up in (0, 1):
        c = m.bits(up, fn, F, bits)
        on = (on_u if up else on_d)
        assert (c[on] != bits[on]).any(axis=-1).all() and np.array_equal(c[~on], bits[~on])
        rest = np.setdiff1d(np.arange(148), lcm.POS)
        assert len(rest) == 34 and np.array_equal(c[..., rest], bits[..., rest])
        assert np.array_equal(m.bits(up, fn, F, c), bits)
    # soft values 0.0 / 1.0 of ciphered bits come back as the plain bits'; NaN stays where it was
    c = m.bits(1, fn, F, bits)
    T = 8 * F
    row = np.arange(T * 2, dtype=np.int32).reshape(T, 2)
    soft = c.transpose(1, 0, 2).reshape(T * 2, 148).astype(np.float32)
    soft[7, 30] = np.nan
    back = m.soft(1, fn, row, np.ones(T * 2, np.uint8), soft)
    want = bits.transpose(1, 0, 2).reshape(T * 2, 148).astype(np.float32)
    want[7, 30] = np.nan
    assert np.array_equal(back, want, equal_nan=True)


@pytest.mark.parametrize("fn0", [0, 1326 * 7 - 50, HYPER - 60])
def test_routing_is_what_the_encoders_write(fn0):
    """On the small plan, every slot the downlink (l1_mux_model) and uplink (l1_ms_model) encoders' walks write for TCH or XCCH
    channel c is routed to (cls, c), and no other slot is routed anywhere: beacon, CCCH, RACH, idle and empty slots are nobody's."""
    comb, F = small_plan(), 208
    m = lcm.CiphModel(comb)
    enc = (lmm.MuxModel(comb, 1, oracle=object()), lms.MsModel(comb, 1, oracle=object()))
    for up in (0, 1):
        cls, chan = m.route(up, fn0, F)
        want_cls, want_chan = np.full_like(cls, -1), np.full_like(chan, -1)
        for c in (lcm.TCH, lcm.XCCH):
            assert len(enc[up].ch[c]) == len(m.ch[c]) == (2 if c == lcm.TCH else 26)
            for i, ch in enumerate(enc[up].ch[c]):
                for k, _ in enc[up].walk(ch.m, fn0, F):
                    assert want_cls[ch.a, 8 * k + ch.tn] == -1
                    want_cls[ch.a, 8 * k + ch.tn], want_chan[ch.a, 8 * k + ch.tn] = c, i
        assert np.array_equal(cls, want_cls) and np.array_equal(chan, want_chan), up
        assert (cls[0, 0::8] == -1).sum() > 50               # combination V: the beacon / CCCH (down), the RACH (up)
        idle = (cls[1, 0::8] == -1)                          # combination I: the idle frame, one in 26
        assert idle.sum() == F // 26 and (cls[1, 0::8] == lcm.XCCH).sum() == F // 26
        assert (cls[:, 3::8] == -1).all()                    # an empty slot
