"""The packet data channel object's statement (tests/l1_pdch_model.py) held to what include/trxsig_l1pdch.h says of it, without a
GPU: frame ownership, the block counts, trxsig_pdch_map_host's table, split-invariance of the encoder and the decoder (outputs
and record bytes) over a cut set that touches every kind of boundary, the hyperframe wrap, the closed loop of the model on
itself, missing bursts, the grant -- and the card's closed-loop condition met by the reference's own modulator and detector."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import fecbind
import fectxbind
import l1_pdch_model as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = (1, 3, 4, 5, 12, 13, 25, 26, 38, 39, 51, 52, 64, 90, 91, 104)
F_ALL = 110
COMB = np.array([[5, 13, 1, 7, 0, 1, 0, 13]], np.uint8)      # two packet slots among circuit-switched ones


@pytest.fixture(scope="module")
def o():
    return fecbind.FecOracle()


def model(o, direction, comb=COMB, bsic=0x2B):
    return lp.Model(comb, bsic, direction, o, fectxbind.TSC_BITS)


def col_of(bits, what):
    """An encoder's grid as a noise-free pull: every written slot a valid burst of 0.0 / 1.0."""
    A, T = what.shape
    return dict(valid=np.ascontiguousarray((what != 0).T), soft=np.ascontiguousarray(bits.transpose(1, 0, 2)).astype(np.float32),
                rssi=np.zeros((T, A), np.int64), timing=np.zeros((T, A), np.int64))


def pieces(fn, cuts):
    edges = [0] + sorted(cuts) + [F_ALL]
    return [(fn + a, fn + b) for a, b in zip(edges[:-1], edges[1:])]


def closed_blocks(dec):
    """{(class, channel, closing FN): the block's outputs} of one decode."""
    out = {}
    for name, r in dec.items():
        for ci, j in zip(*np.nonzero(r["fn"] >= 0)):
            out[(name, int(ci), int(r["fn"][ci, j]))] = tuple(np.asarray(r[k][ci, j]).tobytes() for k in
                                                             ("payload", "cs", "cs_dist", "ok", "usf", "nb", "granted"))
    return out


def test_every_frame_has_one_owner():
    for direction, want in ((lp.DOWN, (96, 4, 4)), (lp.UP, (96, 0, 8))):
        own = [lp.owner(direction, fn) for fn in range(104)]
        count = [sum(x is not None and x[0] == cls for x in own) for cls in (lp.PDTCH, lp.PTCCH)] + [own.count(None)]
        assert tuple(count) == want and sum(count) == 104
        assert [fn for fn in range(104) if own[fn] is None] == ([25, 51, 77, 103] if direction == lp.DOWN else
                                                                [12, 25, 38, 51, 64, 77, 90, 103])
    for base in (0, 52):
        blocks = [lp.owner(lp.DOWN, base + fn) for fn in range(52)]
        assert sorted({x[1] for x in blocks if x and x[0] == lp.PDTCH}) == list(range(12))       # 12 blocks per 52 frames
        for b in range(12):
            assert [x[2] for x in blocks if x and x[:2] == (lp.PDTCH, b)] == [0, 1, 2, 3]
    assert [lp.owner(lp.DOWN, fn)[2] for fn in (12, 38, 64, 90)] == [0, 1, 2, 3]                 # one PTCCH block per 104
    for cls in (lp.PDTCH, lp.PTCCH):                                                             # positions and frames invert
        n = len(lp.FRAMES[cls])
        for q in range(3 * n):
            u = lp.frame_of(cls, q)
            assert lp.pos_before(cls, u) == q and lp.pos_before(cls, u + 1) == q + 1
            assert lp.owner(lp.DOWN, u)[0] == cls
    assert lp.HYPER % 104 == 0 and lp.N_ABS[0] % lp.RING == 0


def test_map_agrees_with_the_library():
    lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", "libtrxsig.so"))
    lib.trxsig_pdch_map_host.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    block, burst = ctypes.c_int(), ctypes.c_int()
    for fn in range(52):
        assert lib.trxsig_pdch_map_host(fn, ctypes.byref(block), ctypes.byref(burst)) == 0
        own = lp.owner(lp.UP, fn)
        assert (block.value, burst.value) == ((own[1], own[2]) if own else (-1, -1)), fn
        if own:
            assert lp.pos_before(lp.PDTCH, fn) == 4 * own[1] + own[2]


def run_split(o, fn, cuts, ins_of, seed):
    """Encode on a DOWN model and decode its bits on another, call by call; -> (grid, what, blocks by closing FN, states)."""
    tx, rx = model(o, lp.DOWN), model(o, lp.DOWN)
    whole = ins_of(tx)
    grids, whats, blocks = [], [], {}
    for f0, f1 in pieces(fn, cuts):
        bits, what = tx.encode(f0 % lp.HYPER, f1 - f0, **lp.slice_inputs(tx, whole, fn, F_ALL, f0, f1))
        grids.append(bits); whats.append(what)
        col = col_of(bits, what)
        keep = np.random.default_rng(seed).random((8 * F_ALL, col["valid"].shape[1])) > 0.2     # the same bursts missing in every split
        col["valid"] &= keep[8 * (f0 - fn):8 * (f1 - fn)]
        got = closed_blocks(rx.decode(col, f0 % lp.HYPER, wire=True, sibling=tx))
        assert not set(got) & set(blocks)
        blocks.update(got)
    return (np.concatenate(grids, axis=1), np.concatenate(whats, axis=1), blocks,
            [m.state(cls).copy() for m in (tx, rx) for cls in (lp.PDTCH, lp.PTCCH)])


@pytest.mark.parametrize("fn", [0, 9, lp.HYPER - 30])
def test_split_invariance(o, fn):
    """One call of 110 frames equals its splits at every single cut, at every pair of cuts and at all of them, in the grid, the
    decoded blocks (by closing FN) and both objects' record bytes.  (fn = 2715648 - 30 crosses the hyperframe, which 52 and
    104 divide.)  Every one of the 2^16 subsets would only repeat these: a call's result depends on the state it starts
    from and on its own frames, and every (cut before, cut after) pair of neighbours occurs among the pairs."""
    rng = np.random.default_rng(fn % 1000)
    ref = model(o, lp.DOWN)
    ins = lp.random_inputs(rng, ref, fn, F_ALL)
    whole = run_split(o, fn, (), lambda m: ins, 5)
    assert whole[1].any() and len(whole[2]) >= 2 * 25
    assert any(np.frombuffer(v[5], np.uint8)[0] not in (0, 4) for v in whole[2].values())          # partial blocks are in play
    splits = [(c,) for c in CUTS] + list(itertools.combinations(CUTS, 2)) + [CUTS]
    for cuts in splits:
        got = run_split(o, fn, cuts, lambda m: ins, 5)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]), cuts
        assert got[2] == whole[2], cuts
        for g, w in zip(got[3], whole[3]):
            assert np.array_equal(g, w), cuts
    if fn > lp.HYPER // 2:
        fns = sorted(k[2] for k in whole[2])
        assert fns[0] < 110 and fns[-1] > lp.HYPER - 30                                            # closing FNs wrapped


def test_model_loop_returns_every_block(o):
    """encode -> bits as 0.0 / 1.0 soft rows -> decode: every payload, scheme and USF, ok = 1, nb = 4; what was not sent closes with
    nb = 0; granted = the USF of the previous absolute block, 255 across a gap and without a sibling."""
    fn, F = 9, 104 + 13                                         # 27 blocks: the ring of 32 keeps them all
    rng = np.random.default_rng(3)
    tx, rx, rx2 = model(o, lp.DOWN), model(o, lp.DOWN), model(o, lp.DOWN)
    ins = lp.random_inputs(rng, tx, fn, F, p_send=0.7)
    bits, what = tx.encode(fn, F, **ins)
    assert set(np.unique(what)) == {0, lp.WHAT_PDCH} and not what[:, [i for i in range(8 * F) if i % 8 not in (1, 7)]].any()
    dec = rx.decode(col_of(bits, what), fn, wire=True, sibling=tx)
    none = rx2.decode(col_of(bits, what), fn, wire=True, sibling=None)
    assert (none["pdtch"]["granted"] == 255).all() and (dec["ptcch"]["granted"] == 255).all()
    bf, nb = lp.encode_blocks(lp.PDTCH, fn, F)
    blk0, shown, nclose = lp.decode_blocks(lp.PDTCH, fn, F)
    assert bf == blk0 + 1 and shown == nb + 1                    # fn = 9 is inside B2: it shows, with no burst, and closes
    r = dec["pdtch"]
    sent = (ins["kind"] == 1) & (ins["cs"] <= 3)
    assert sent.any() and not sent.all()
    seen_gap = seen_grant = False
    for ci in range(len(tx.chan[lp.PDTCH])):
        assert r["nb"][ci, 0] == 0 and r["ok"][ci, 0] == 0 and r["cs"][ci, 0] == 255 and r["fn"][ci, 0] == 11
        for b in range(nb):
            j = b + 1
            if j >= nclose:
                assert r["fn"][ci, j] == -1
                continue
            if sent[ci, b]:
                assert (r["ok"][ci, j], r["nb"][ci, j], r["cs"][ci, j], r["cs_dist"][ci, j]) == (1, 4, ins["cs"][ci, b], 0)
                assert np.array_equal(r["payload"][ci, j], ins["payload"][ci, b]) and r["usf"][ci, j] == ins["payload"][ci, b, 0] & 7
            else:
                assert (r["ok"][ci, j], r["nb"][ci, j], r["cs"][ci, j], r["usf"][ci, j]) == (0, 0, 255, 255)
                assert not r["payload"][ci, j].any()
            if b > 0:
                want = ins["payload"][ci, b - 1, 0] & 7 if sent[ci, b - 1] else 255
                assert r["granted"][ci, j] == want
                seen_gap |= want == 255
                seen_grant |= want != 255
    assert seen_gap and seen_grant
    pt = dec["ptcch"]
    assert pt["fn"].shape[1] == 2 and (pt["fn"][:, 0] == 90).all()
    for ci in range(len(tx.chan[lp.PTCCH])):
        if ins["pt_kind"][ci, 0]:
            assert pt["ok"][ci, 0] == 1 and pt["cs"][ci, 0] == 0 and np.array_equal(pt["payload"][ci, 0], ins["pt_payload"][ci, 0])


def test_missing_bursts_are_counted(o):
    fn, F = 0, 52
    rng = np.random.default_rng(4)
    tx, rx = model(o, lp.UP), model(o, lp.UP)
    ins = lp.random_inputs(rng, tx, fn, F, p_send=1.1)
    ins["cs"][:] = np.arange(12) % 4
    bits, what = tx.encode(fn, F, **ins)
    col = col_of(bits, what)
    tn = tx.chan[lp.PDTCH][0][1]
    gone = {0: [], 1: [2], 2: [0, 1, 3], 3: [0, 1, 2, 3], 4: [3]}            # block -> bursts removed
    for b, ts in gone.items():
        for t in ts:
            col["valid"][8 * lp.frame_of(lp.PDTCH, 4 * b + t) + tn, 0] = False
    r = rx.decode(col, fn, wire=False)["pdtch"]
    assert [int(r["nb"][0, b]) for b in range(5)] == [4, 3, 1, 0, 3] and (r["nb"][1] == 4).all()
    assert r["ok"][0, 0] == 1 and r["ok"][0, 3] == 0 and r["cs"][0, 3] == 255 and (r["fn"][0] == [3, 7, 11, 16, 20, 24, 29, 33, 37, 42, 46, 50]).all()
    assert r["cs"][0, 1] == ins["cs"][0, 1] and r["cs"][0, 4] == ins["cs"][0, 4]      # seven and six of the eight flags still vote
    assert (what[:, 8 * 12:8 * 13] == 0).all() and (what[:, 8 * 38:8 * 39] == 0).all()   # an UP object leaves 12 and 38 alone


def test_reference_detector_meets_the_closed_loop_condition(o):
    """What tests/test_gpu_l1pdch.py asks of the card's closed loop -- 30 noise-free frames, every block sent back ok, every other
    one empty -- through the reference's modulator, midamble detector and demodulator on the CPU."""
    import oraclebind
    so = oraclebind.Oracle(4)
    fn, F = 9, 30
    rng = np.random.default_rng(6)
    tx, rx = model(o, lp.UP), model(o, lp.UP)
    ins = lp.random_inputs(rng, tx, fn, F, p_send=0.75)
    bits, what = tx.encode(fn, F, **ins)
    col = col_of(bits, what)
    for slot, a in zip(*np.nonzero(what.T)):
        x = so.modulate(bits[a, slot], 8 + (slot % 4 == 0))
        d = so.analyze_traffic(x, tx.tsc)
        col["valid"][slot, a] = d["ok"]
        col["soft"][slot, a] = so.demodulate(x, d["amp"], d["toa"])[:148]
    assert col["valid"].sum() == (what != 0).sum()
    r = rx.decode(col, fn, wire=True)["pdtch"]
    bf, nb = lp.encode_blocks(lp.PDTCH, fn, F)
    blk0, shown, nclose = lp.decode_blocks(lp.PDTCH, fn, F)
    sent = (ins["kind"] == 1) & (ins["cs"] <= 3)
    assert sent.sum() >= 8 and len(set(ins["cs"][sent])) == 4
    for ci in range(sent.shape[0]):
        for b in range(nb):
            j = b + bf - blk0
            if sent[ci, b] and j < nclose:
                assert (r["ok"][ci, j], r["cs"][ci, j], r["usf"][ci, j]) == (1, ins["cs"][ci, b], ins["payload"][ci, b, 0] & 7)
                assert np.array_equal(r["payload"][ci, j], ins["payload"][ci, b])
            elif not sent[ci, b]:
                assert r["nb"][ci, j] == 0
