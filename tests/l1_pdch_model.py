"""Packet data channels through L1 (include/trxsig_l1pdch.h) in numpy -- TEST INFRASTRUCTURE ONLY.  The block coders are
tests/pdtch_model.py's and the 52-multiframe is its pdch_map; what is stated here is what the object adds: which frame belongs to
whom, how blocks are numbered in an encode call (trxsig_l1tx's rule) and in a decode call (trxsig_l1rx's), the encoder with its
pending bursts and USF ring, the decoder with its carried rows, d_nb, closing FN and the grant, and the channel record's bytes.

The PTCCH/D positions (FN mod 104 = 12, 38, 64, 90) are written from memory of GSM 05.02 (the header says so)."""
import numpy as np

import pdtch_model as pm
from l1_demux_model import wire_phy

HYPER = 2048 * 26 * 51
DOWN, UP = 0, 1
PDTCH, PTCCH = 0, 1
COMB = 13
WHAT_PDCH = 8
RING = 32
PERIOD = (52, 104)
FRAMES = (tuple(f for f in range(52) if pm.pdch_map(f)[0] >= 0), (12, 38, 64, 90))
N_ABS = (12 * (HYPER // 52), HYPER // 104)                   # absolute block numbers wrap here
OCTETS = (54, 23)
STATE = np.dtype([("pend_blk", "<i4"), ("carry_blk", "<i4"), ("carry_have", "<u4"), ("pad", "<i4"), ("bits", "u1", (4, 148)),
                  ("ring", "<i4", (RING,)), ("carry", "<f4", (4, 148))])
assert STATE.itemsize == 3104                                # TRXSIG_L1PDCH_STATE_BYTES


def owner(direction, fn):
    """Who owns frame fn of a PDCH: (PDTCH, block 0..11, burst), (PTCCH, 0, burst) or None."""
    if fn % 104 in FRAMES[PTCCH]:
        return (PTCCH, 0, FRAMES[PTCCH].index(fn % 104)) if direction == DOWN else None
    b, t = pm.pdch_map(fn)
    return (PDTCH, b, t) if b >= 0 else None


def pos_before(cls, u):
    """The class's burst frames below (unwrapped) frame u."""
    return len(FRAMES[cls]) * (u // PERIOD[cls]) + sum(f < u % PERIOD[cls] for f in FRAMES[cls])


def frame_of(cls, q):
    n = len(FRAMES[cls])
    return PERIOD[cls] * (q // n) + FRAMES[cls][q % n]


def encode_blocks(cls, fn, F):
    """(first block, count) of the blocks whose first burst is in [fn, fn + F): trxsig_l1tx's rule."""
    bf = -(-pos_before(cls, fn) // 4)
    return bf, -(-pos_before(cls, fn + F) // 4) - bf


def decode_blocks(cls, fn, F):
    """(first block, shown, closing) of the blocks with a burst frame in [fn, fn + F): trxsig_l1rx's rule."""
    pf, pe = pos_before(cls, fn), pos_before(cls, fn + F)
    if pe <= pf:
        return pf // 4, 0, 0
    return pf // 4, (pe - 1) // 4 - pf // 4 + 1, pe // 4 - pf // 4


def circuit_plan(comb):
    comb = np.asarray(comb, np.uint8)
    return np.where(comb == COMB, 0, comb).astype(np.uint8)


class Model:
    def __init__(self, comb, bsic, direction, o, tsc_bits):
        self.comb = np.asarray(comb, np.uint8)
        assert np.isin(self.comb, (0, 1, 5, 7, COMB)).all() and direction in (DOWN, UP)
        self.A, self.dir, self.tsc, self.o, self.tsc_bits = self.comb.shape[0], direction, bsic & 7, o, tsc_bits
        slots = [(a, tn) for a in range(self.A) for tn in range(8) if self.comb[a, tn] == COMB]
        self.chan = (slots, slots if direction == DOWN else [])
        self.st = [np.zeros(len(c), STATE) for c in self.chan]
        for s in self.st:
            s["pend_blk"] = s["carry_blk"] = -1
            s["ring"] = -1
        self.rssi = [np.zeros(len(c), np.int32) for c in self.chan]
        self.timing = [np.zeros(len(c), np.int32) for c in self.chan]

    def grid(self, fn, F):
        return tuple(encode_blocks(cls, fn, F)[1] if self.chan[cls] else 0 for cls in (PDTCH, PTCCH))

    def state(self, cls):
        return self.st[cls].view(np.uint8).reshape(len(self.chan[cls]), STATE.itemsize)

    def encode(self, fn, F, kind=None, cs=None, payload=None, pt_kind=None, pt_payload=None, onto=None):
        """kind / cs [n][nb], payload [n][nb][54]; pt_kind [n][nb_pt], pt_payload [n][nb_pt][23] -> (bits [A][8 F][148], what
        [A][8 F]); onto: (bits, what) to overlay (copied)."""
        if onto is None:
            bits, what = np.zeros((self.A, 8 * F, 148), np.uint8), np.zeros((self.A, 8 * F), np.uint8)
        else:
            bits, what = onto[0].copy(), onto[1].copy()
        for cls in (PDTCH, PTCCH):
            bf, nb = encode_blocks(cls, fn, F)
            pe = pos_before(cls, fn + F)
            for ci, (a, tn) in enumerate(self.chan[cls]):
                S = self.st[cls][ci]
                coded = {}                                   # block -> its four bursts, for the blocks sent
                for b in range(nb):
                    c = int(cs[ci][b]) if cls == PDTCH else pm.CS1
                    k = (kind if cls == PDTCH else pt_kind)[ci][b]
                    if k != 1 or c > 3:
                        continue
                    pl = np.zeros(54, np.uint8)
                    pl[:OCTETS[cls]] = (payload if cls == PDTCH else pt_payload)[ci][b]
                    coded[bf + b] = pm.encode(self.o, pl[None], [c], [self.tsc], self.tsc_bits)[0]
                    if cls == PDTCH and self.dir == DOWN:
                        n = (bf + b) % N_ABS[cls]
                        S["ring"][n % RING] = n << 8 | (int(pl[0]) & 7)
                if S["pend_blk"] >= 0 and bf > 0 and S["pend_blk"] == (bf - 1) % N_ABS[cls]:
                    coded[bf - 1] = S["bits"].copy()
                for k in range(F):
                    u = fn + k
                    own = owner(self.dir, u)
                    if own is None or own[0] != cls:
                        continue
                    q = pos_before(cls, u)
                    if q // 4 in coded:
                        bits[a, 8 * k + tn] = coded[q // 4][q % 4]
                        what[a, 8 * k + tn] = WHAT_PDCH
                S["pend_blk"], S["bits"] = -1, 0
                if pe % 4 and pe // 4 in coded:                  # the block that straddles the call's end
                    S["pend_blk"], S["bits"] = (pe // 4) % N_ABS[cls], coded[pe // 4]
        return bits, what

    def decode(self, col, fn, wire=True, cs_force=-1, sibling=None):
        """col: dict(valid [8 F][A], soft [8 F][A][148], rssi, timing [8 F][A]) of whole frames from (fn, TN 0), as
        trxsig_trxgroup_collect reports a pull.  -> {"pdtch": ..., "ptcch": ...}, each dict(payload, cs, cs_dist, ok, usf, nb,
        granted, fn, rssi, timing)."""
        valid, soft = np.asarray(col["valid"]), np.asarray(col["soft"], np.float32)
        F = valid.shape[0] // 8
        out = {}
        for cls, name in ((PDTCH, "pdtch"), (PTCCH, "ptcch")):
            n = len(self.chan[cls])
            blk0, nb, nclose = decode_blocks(cls, fn, F) if n else (0, 0, 0)
            pf, pe = pos_before(cls, fn), pos_before(cls, fn + F)
            r = dict(payload=np.zeros((n, nb, OCTETS[cls]), np.uint8), ok=np.zeros((n, nb), np.uint8), nb=np.zeros((n, nb), np.uint8),
                     fn=np.full((n, nb), -1, np.int32), **{k: np.full((n, nb), 255, np.uint8) for k in ("cs", "cs_dist", "usf", "granted")})
            for ci, (a, tn) in enumerate(self.chan[cls]):
                S = self.st[cls][ci]
                carried = {}
                if S["carry_blk"] >= 0 and S["carry_blk"] == blk0 % N_ABS[cls]:
                    carried = {t: S["carry"][t].copy() for t in range(4) if S["carry_have"] >> t & 1}
                last_open = None
                for j in range(nb):
                    blk = blk0 + j
                    rows = {}
                    for t in range(4):
                        q = 4 * blk + t
                        if q >= pe:
                            continue
                        if q < pf:
                            if t in carried:
                                rows[t] = carried[t]
                            continue
                        k = frame_of(cls, q) - fn
                        if valid[8 * k + tn, a]:
                            rows[t] = soft[8 * k + tn, a, :148].copy()
                            self.rssi[cls][ci], self.timing[cls][ci] = wire_phy(col["rssi"][8 * k + tn, a], col["timing"][8 * k + tn, a])
                    r["nb"][ci, j] = len(rows)
                    if cls == PDTCH and sibling is not None:
                        m = (blk - 1) % N_ABS[cls]
                        ent = int(sibling.st[PDTCH][ci]["ring"][m % RING])
                        if ent >= 0 and ent >> 8 == m:
                            r["granted"][ci, j] = ent & 255
                    if j >= nclose:
                        last_open = (blk, rows)
                        continue
                    r["fn"][ci, j] = frame_of(cls, 4 * blk + 3) % HYPER
                    if not rows:
                        continue
                    v4 = np.full((4, 148), 0.5, np.float32)
                    for t, v in rows.items():
                        v4[t] = self.o.wire(v) if wire else v
                    d = pm.decode_block(self.o, v4, cs_force if cls == PDTCH else pm.CS1)
                    r["payload"][ci, j] = d["block"][:OCTETS[cls]]
                    r["cs"][ci, j], r["cs_dist"][ci, j], r["ok"][ci, j], r["usf"][ci, j] = d["cs"], d["dist"], d["ok"], d["usf"]
                if nb:                                           # a call without a burst frame leaves the carry as it is
                    S["carry_blk"], S["carry_have"], S["carry"] = -1, 0, 0
                    if last_open is not None:
                        S["carry_blk"] = last_open[0] % N_ABS[cls]
                        for t, v in last_open[1].items():
                            S["carry_have"] |= 1 << t
                            S["carry"][t] = v
            r["rssi"], r["timing"] = self.rssi[cls].copy(), self.timing[cls].copy()
            out[name] = r
        return out


def random_inputs(rng, model, fn, F, p_send=0.8):
    """Encode inputs of a call: schemes mixed inside a channel, some blocks not sent (kind 0 or 2, cs 4 or 255)."""
    nb, nbt = model.grid(fn, F)
    n, nt = len(model.chan[PDTCH]), len(model.chan[PTCCH])
    cs = rng.integers(0, 4, (n, nb)).astype(np.uint8)
    payload = pm.random_blocks(rng, cs.reshape(-1)).reshape(n, nb, 54)
    kind = np.where(rng.random((n, nb)) < p_send, 1, rng.choice(np.array([0, 2], np.uint8), (n, nb))).astype(np.uint8)
    bad = rng.random((n, nb)) < 0.1
    cs[bad] = rng.choice(np.array([4, 255], np.uint8), int(bad.sum()))
    pt_kind = (rng.random((nt, nbt)) < p_send).astype(np.uint8)
    pt_payload = rng.integers(0, 256, (nt, nbt, 23)).astype(np.uint8)
    return dict(kind=kind, cs=cs, payload=payload, pt_kind=pt_kind, pt_payload=pt_payload)


def slice_inputs(model, ins, fn, F, f0, f1):
    """The part of a whole call's inputs [fn, fn + F) that the call [f0, f1) takes."""
    out = {}
    for cls, keys in ((PDTCH, ("kind", "cs", "payload")), (PTCCH, ("pt_kind", "pt_payload"))):
        b0 = encode_blocks(cls, f0, f1 - f0)[0] - encode_blocks(cls, fn, F)[0]
        nb = encode_blocks(cls, f0, f1 - f0)[1] if model.chan[cls] else 0
        for k in keys:
            out[k] = np.ascontiguousarray(ins[k][:, b0:b0 + nb])
    return out
