"""The model of the hopping stage (tests/l1_hop_model.py): RNTABLE's checks, the two known answers (which pin this project's
reading of GSM 05.02 6.2.3, not the standard: it publishes no vector), the sequence's properties for every N, the operations'
own identities, and on the CPU what hopping is for: SDCCH channels that keep decoding while one frequency is lost.  No GPU."""
import os
import re
import zlib

import numpy as np
import pytest

import fec_stream_model as fsm
import l1_hop_model as lhm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = lhm.HYPERFRAME
KNOWN = (((1, 0, 4), range(0, 20), [2, 0, 3, 2, 3, 3, 2, 0, 1, 1, 2, 3, 1, 1, 1, 3, 3, 1, 0, 0]),
         ((63, 2, 64), range(83578, 83590), [47, 41, 7, 57, 45, 9, 6, 52, 35, 34, 35, 11]))


def test_table():
    t = lhm.RNTABLE
    assert len(t) == 114 and len(set(t)) == 114 and max(t) <= 127 and min(t) == 0
    assert sorted(set(range(128)) - set(t)) == [10, 14, 20, 27, 28, 30, 35, 41, 44, 50, 69, 83, 115, 116]
    assert sum(t) == 7446
    assert zlib.crc32(bytes(t)) == 0xED53E222


def test_known_answers():
    for (hsn, maio, n), fns, want in KNOWN:
        assert [lhm.mai(fn, hsn, maio, n) for fn in fns] == want
    assert 83578 // 1326 == 63


def test_cyclic_and_single():
    rng = np.random.default_rng(1)
    for fn in list(rng.integers(0, HYPER, 300)) + [0, HYPER - 1]:
        n = int(rng.integers(1, 65))
        maio = int(rng.integers(0, n))
        assert lhm.mai(fn, 0, maio, n) == (int(fn) + maio) % n
        assert lhm.mai(fn, int(rng.integers(0, 64)), 0, 1) == 0


def frames():
    rng = np.random.default_rng(2)
    edge = [83577, 83578, 83579, 84863, 84864, 84865, HYPER - 1, 0, 1, 1325, 1326]      # T1R 62 -> 63, 63 -> 0, the wrap
    return edge + list(range(40000, 41400)) + [int(x) for x in rng.integers(0, HYPER, 1500)]


@pytest.mark.parametrize("hsn", [0, 1, 17, 63])
def test_every_n(hsn):
    """MAI < N; the N MAIOs of a frame give a permutation (a rotation); for N = 64 the branch M' >= N is taken."""
    fns = frames()
    assert len(fns) > 2900 and 84863 // 1326 % 64 == 63 and 84864 // 1326 % 64 == 0
    for n in range(1, 65):
        took = []
        for fn in fns:
            s = lhm.s_of(fn, hsn, n, took)
            assert 0 <= s < n
            if n <= 8 or fn % 97 == 0:                        # the permutation, spelled out
                m = [lhm.mai(fn, hsn, maio, n) for maio in range(n)]
                assert sorted(m) == list(range(n)) and m == [(s + k) % n for k in range(n)]
        if hsn and n == 64:
            assert any(took) and not all(took)
        if hsn and n > 1:
            assert len({lhm.s_of(fn, hsn, n) for fn in fns[:400]}) == n      # every frequency is visited


plan = lhm.small_plan


def test_plan_rules():
    comb, group, hsn = plan()
    m = lhm.HopModel(comb, group, hsn)
    assert m.groups() == 4 and m.members(0, 1) == [0, 2, 5] and m.members(1, 2) == [3] and m.members(1, 4) == [0, 1, 3]
    assert m.members(3, 4) == [2, 5] and m.members(3, 0) == []
    bad = []
    g = group.copy(); g[0, 0] = 0; bad.append((comb, g, hsn))                           # the beacon slot
    g = group.copy(); g[6, 1] = 0; bad.append((comb, g, hsn))                           # an OFF slot
    c = comb.copy(); c[2, 1] = 1; bad.append((c, group, hsn))                           # members differ
    g = group.copy(); g[1, 2] = 4; bad.append((comb, g, hsn))                           # group id out of range
    g = group.copy(); g[1, 2] = -2; bad.append((comb, g, hsn))
    bad.append((comb, group, np.array([5, 0, 64, 17])))                                # HSN
    c65, g65 = np.ones((65, 8), np.uint8), np.full((65, 8), -1, np.int8)
    g65[:, 6] = 0
    bad.append((c65, g65, [1]))                                                        # N = 65
    for b in bad:
        with pytest.raises(ValueError):
            lhm.HopModel(*b)
    g65[64, 6] = -1
    assert len(lhm.HopModel(c65, g65, [1]).members(0, 6)) == 64


def test_operations():
    rng = np.random.default_rng(4)
    comb, group, hsn = plan()
    m = lhm.HopModel(comb, group, hsn)
    A, F, fn = 7, 12, HYPER - 5
    T = 8 * F
    radio = m.map(fn, F)
    assert radio.shape == (T, A) and (np.sort(radio, axis=1) == np.arange(A)).all()      # a permutation of the rows in every slot
    fixed = group.T[np.arange(T) % 8] < 0                    # [T][A]
    assert (radio[fixed] == np.broadcast_to(np.arange(A), (T, A))[fixed]).all()
    assert radio[2::8, 3].tolist() == [3] * F              # N = 1 stays
    assert (radio != np.arange(A)).sum() > 50                # of the 9 x 12 slots of groups with N > 1
    for g, tn in ((0, 1), (2, 3), (1, 4), (3, 4)):           # a group's rows stay among themselves
        rows = m.members(g, tn)
        assert set(radio[tn::8][:, rows].ravel()) == set(rows)
    bits = rng.integers(0, 2, (A, T, 148)).astype(np.uint8)
    what = rng.integers(0, 8, (A, T)).astype(np.uint8)
    b1, w1 = m.bits(1, fn, F, bits, what)
    assert not np.array_equal(b1, bits) and np.array_equal(b1[radio.T, np.arange(T)[None, :]], bits)
    b0, w0 = m.bits(0, fn, F, b1, w1)
    assert np.array_equal(b0, bits) and np.array_equal(w0, what)
    assert m.bits(1, fn, F, bits)[1] is None
    # one call equals a split at a frame boundary (across the hyperframe wrap)
    lo, lw = m.bits(1, fn, 5, bits[:, :40], what[:, :40])
    hi, hw = m.bits(1, (fn + 5) % HYPER, 7, bits[:, 40:], what[:, 40:])
    assert np.array_equal(np.concatenate([lo, hi], 1), b1) and np.array_equal(np.concatenate([lw, hw], 1), w1)
    assert np.array_equal(np.concatenate([m.map(fn, 5), m.map((fn + 5) % HYPER, 7)]), radio)
    # result: the entry of the radio row; cells: the same move as bits
    row = rng.integers(-1, 500, (T, A)).astype(np.int32)
    out = m.result(fn, row)
    assert all(out[t, a] == row[t, radio[t, a]] for t in range(T) for a in range(A))
    sps, cell = 1, 160
    src = rng.integers(1, 1 << 62, T * A * cell).astype(np.uint64)
    dst = np.zeros_like(src)
    m.cells(1, fn, F, src, A * cell, cell, dst, cell, T * cell, sps)
    for t in (0, 9, 35, T - 1):
        n = lhm.cell_len(t, sps)
        for a in range(A):
            o = t * cell + int(radio[t, a]) * T * cell
            assert np.array_equal(dst[o:o + n], src[t * A * cell + a * cell:][:n]) and not dst[o + n:o + cell].any()
    back = np.zeros_like(src)
    m.cells(0, fn, F, dst, cell, T * cell, back, A * cell, cell, sps)
    keep = np.zeros(T * A * cell, bool)
    for t in range(T):
        for a in range(A):
            keep[(t * A + a) * cell:][:lhm.cell_len(t, sps)] = True
    assert np.array_equal(back[keep], src[keep]) and not back[~keep].any()


def sdcch8_uplink():
    """the uplink SDCCH/8 mappings of csrc/trxsig_tdma.h: (repeat length, frames) of sub-channels 0..7"""
    h = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_tdma.h")).read()
    body = h[h.index("#define TRX_TDMA_MAPS_INIT"):h.index("constexpr int kTrxHyperframe")]
    m4 = [tuple(int(x) for x in e) for e in re.findall(r"TRX_M4\((\d+), (\d+), (\d+), (\d+), (\d+)\)", body)]
    assert len(m4) == 32                                     # ids 1..32; id 0 and id 33 are written out
    maps = m4[8:16]                                          # TRX_MAP_SDCCH8 = 9
    assert all(r == 51 for r, *_ in maps) and maps[0][1:] == (15, 16, 17, 18) and maps[7][1:] == (43, 44, 45, 46)
    return [(r, f) for r, *f in maps]


def test_hopping_keeps_sdcch_alive_when_a_frequency_is_lost():
    """Four combination-VII rows in one group on TN 2, HSN 0 (cyclic), radio row 1 never arriving.  Twelve blocks of each of the
    32 SDCCH channels through the reference's XCCH encoder and the stream decoder's model, noise 0.  What decodes is read off the
    decoder's rules (fec_stream_model): a block is decoded only when its closing burst arrives; a row whose burst did not
    arrive holds 0.5 (an erasure) only if a deinterleave has happened since it last held data, else another block's values or
    a fresh decoder's 0.0.  So a block whose closing burst is lost has status 0; a block whose closing burst arrives and whose
    other rows hold its own bursts or erasures decodes to its frame (one erased burst in four never failed in 1,200 trials at
    noise 0); a block with a stale row almost never passes parity (7 of 2,400 trials), and where it does it is its frame: no
    claim is made on those.  With the group switched off the channels of row 1 decode nothing and the others everything."""
    prims = fsm.Prims()
    rng = np.random.default_rng(7)
    A, tn, nb, lost = 4, 2, 12, 1
    comb = np.zeros((A, 8), np.uint8); comb[:, tn] = 7
    group = np.full((A, 8), -1, np.int8); group[:, tn] = 0
    maps = sdcch8_uplink()
    fn0, F = 51 * 26 * 3, 51 * nb                            # a multiple of 51: block k of sub s is frames fn0 + 51 k + f[0..3]
    S = A * 8
    soft, frames_sent = fsm.xcch_bursts(rng, prims.fo, S, nb, noise=0.0)      # [S][4 nb][148]
    state = np.zeros((S, fsm.XCCH_STATE_BYTES), np.uint8)
    runs = {}
    for hop in (True, False):
        m = lhm.HopModel(comb, group if hop else np.full_like(group, -1), [0])
        radio = m.map(fn0, F)
        # the radio domain: a pull's row per (slot, radio row), -1 on the lost frequency; the rows' soft values by channel
        T = 8 * F
        row = np.arange(T * A, dtype=np.int32).reshape(T, A)
        row[:, lost] = -1
        rows = np.zeros((T * A, 148), np.float32)
        index = np.full((S, 4 * nb), -1, np.int64)
        want = np.zeros((S, nb), bool)                       # must decode
        closed = np.zeros((S, nb), bool)                     # the closing burst arrives
        closing = [set() for _ in range(S)]
        dehopped = m.result(fn0, row)                        # [T][A] in the channel domain
        for a in range(A):
            for s, (R, f) in enumerate(maps):
                ch = a * 8 + s
                held = ["zeros"] * 4                         # what each of the decoder's four rows holds
                for k in range(nb):
                    for j in range(4):
                        t = 8 * (51 * k + f[j]) + tn
                        r = int(radio[t, a])
                        rows[t * A + r] = soft[ch, 4 * k + j]
                        index[ch, 4 * k + j] = dehopped[t, a]
                        if r != lost:
                            held[j] = k
                        if j == 3:
                            closing[ch].add(r)
                            if r != lost:
                                closed[ch, k] = True
                                want[ch, k] = all(h in (k, "erased") for h in held)
                                held = ["erased"] * 4
        assert (index >= -1).all() and (np.sort(index[index >= 0]) == np.unique(index[index >= 0])).all()
        out = fsm.run(prims, False, rows, index, state)
        good = out["status"] == (fsm.DECODED | fsm.TCH_GOOD)
        assert good[want].all() and np.array_equal(out["status"] != 0, closed)
        assert np.array_equal(out["l2"][good], frames_sent[good])
        runs[hop] = (good, closing)
    good, closing = runs[True]
    assert all(len(c) == 4 for c in closing)                 # every channel's closing bursts visit more than one frequency
    assert (good.sum(axis=1) >= 4).all() and not good.all(axis=1).any()      # every channel decodes some of its blocks
    flat, closing = runs[False]
    on_lost = np.arange(S) // 8 == lost
    assert not flat[on_lost].any() and flat[~on_lost].all()
    assert all(closing[ch] == {ch // 8} for ch in range(S))
    assert good[on_lost].any(axis=1).all()                   # the same channels, hopping
