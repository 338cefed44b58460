"""A literal model of the mobile-side uplink L1 (trxsig_l1ms.h) on the CPU -- TEST INFRASTRUCTURE ONLY.

  the walk:                     each handset encoder walks its UPLINK TDMAMapping frame by frame exactly as the downlink's do
                                (l1_mux_model.MuxModel.walk over the tables of tests/golden/tdma_uplink.npz, loaded by
                                l1_demux_model.load_mappings); a burst's B is reverseMapping(FN) % 4, a block starts at B == 0
  XCCHL1Encoder::sendFrame:     the oracle's fo_xcch_encode (TSC = BCC); kind != 1 sends nothing (no uplink idle fill)
  the SACCH L1 header:          octet 0 = encodePower(actual power), octet 1 = actual TA -- what SACCHL1Decoder::handleGoodFrame
                                reads back (mU.peekField(3, 5), peekField(9, 7))
  TCHFACCHL1Encoder::dispatch:  the oracle's fo_tch_encode_stream, its 32-byte state chained block to block
  the access burst:             GSM 05.02 5.2.7 (extended tail, synch sequence) around the 36 coded bits of GSM 05.03 4.6, the
                                inverse of RACHL1Decoder::writeLowSide (tests/test_gpu_l1rx.py::rach_e36's rule)
  the handsets:                 per SACCH channel the actual power / TA; with a sibling L1Tx, its current orders as the header it
                                writes decodes them, taken once at the start of the call by every open SACCH channel

Outputs are laid out as the library lays them out: bits [n_arfcn][8 F][148], what [n_arfcn][8 F], who [n_arfcn][8 F] (the slot's
channel within its class, or its RACH entry; -1 empty), the handsets per XCCH channel, and the channels' 160-byte records."""
import numpy as np

import fecbind
import fectxbind
import l1_demux_model as ldm
import l1_mux_model as lmm

HYPERFRAME = lmm.HYPERFRAME
TCH, XCCH, RACH = 0, 1, 2
W_NONE, W_TCH, W_XCCH, W_ACCESS = range(4)
STATE_BYTES = 160
POWER = lmm.POWER
ACCESS_HEAD = np.array([int(ch) for ch in "00111010" "01001011011111111001100110101010001111000"], np.uint8)   # GSM 05.02 5.2.7

_K = np.arange(456)
_J = 2 * ((49 * _K) % 57) + ((_K % 8) // 4)                 # GSM 05.03 3.1.3 / 4.1.4
_E = np.r_[3:60, 88:145]                                     # the burst's e-bit positions


def load_mappings():
    """The uplink tables, as the Mapping the downlink model's walk takes."""
    return {n: lmm.Mapping(n, m.R, m.frames) for n, m in ldm.load_mappings().items()}


def level_power(band, power):
    """POWER[band][encodePower(band, power)]: the band's level nearest the ordered power"""
    return POWER[band][lmm.encode_power(band, int(power))]


def rach_e36(fo, ra, bsic):
    """u[0..7] = RA, LSB first; u[8..13] = ~(bsic ^ parity6(u[0..7])), MSB first; u[14..17] = 0; the rate-1/2 coder."""
    u = np.zeros(18, np.uint8)
    u[:8] = [(ra >> i) & 1 for i in range(8)]
    p = (~(bsic ^ fo.parity(fecbind.RACH_POLY, 6, u[:8]))) & 0x3F
    u[8:14] = [(p >> (5 - i)) & 1 for i in range(6)]
    return fo.encode(u)


def access_burst(fo, ra, bsic):
    b = np.zeros(148, np.uint8)
    b[:49] = ACCESS_HEAD
    b[49:85] = rach_e36(fo, ra, bsic)
    return b


class Channel:
    def __init__(self, cls, a, tn, mapping, sub):
        self.cls, self.a, self.tn, self.m, self.sub = cls, a, tn, mapping, sub
        self.sacch = mapping.name.startswith("SACCH")
        self.active = True
        self.block = None                                    # bursts [4][148] of the block being sent, or None
        self.left = 0                                        # bursts of it still to go out
        self.tch_state = np.zeros(32, np.uint8)
        self.power = self.ta = -1                            # SACCH channels: the handset
        self.handset = None                                  # the SACCH channel whose handset sends this channel
        self.last_c = np.zeros(456, np.uint8)
        self.prev_c = np.zeros(456, np.uint8)
        self.last_f = self.prev_f = 0

    def record(self):
        r = np.zeros(STATE_BYTES, np.uint8)
        r[0:57] = np.packbits(self.last_c, bitorder="little")
        r[64:121] = np.packbits(self.prev_c, bitorder="little")
        r[128:132] = [self.last_f, self.prev_f, int(self.block is not None and self.left > 0), int(self.active)]
        r[132:140] = np.array([self.power, self.ta], "<i4").view(np.uint8)
        return r


class MsModel:
    def __init__(self, comb, bsic, band=900, oracle=None, maps=None):
        self.comb = np.asarray(comb, np.uint8)
        self.bsic, self.band = int(bsic), int(band)
        self.o = oracle or fectxbind.FecTxOracle()
        self.maps = M = maps or load_mappings()
        self.tsc = fectxbind.TSC_BITS[self.bsic & 7]
        self.filler = np.zeros(456, np.uint8)
        self.ch = {TCH: [], XCCH: [], RACH: []}
        for a in range(self.comb.shape[0]):
            for tn in range(8):
                k = int(self.comb[a, tn])
                x = self.ch[XCCH]
                if k == 1:
                    t = Channel(TCH, a, tn, M["FACCH_TCHF"], 0)
                    s = Channel(XCCH, a, tn, M["SACCH_TF_T%d" % tn], 0)
                    t.handset = s.handset = s
                    self.ch[TCH].append(t)
                    x.append(s)
                elif k in (5, 7):
                    n, tag = (4, "4") if k == 5 else (8, "8")
                    sd = [Channel(XCCH, a, tn, M["SDCCH_%s_%dU" % (tag, s)], s) for s in range(n)]
                    sa = [Channel(XCCH, a, tn, M["SACCH_C%s_%dU" % (tag, s)], s) for s in range(n)]
                    for d, s in zip(sd, sa):
                        d.handset = s.handset = s
                    x += sd + sa
                    if k == 5:
                        assert a == 0 and tn == 0
                        self.ch[RACH].append(Channel(RACH, a, tn, M["RACHC5"], 0))
                elif k != 0:
                    raise ValueError("unsupported combination")
        for c in self.ch[XCCH]:
            if c.sacch:
                c.power, c.ta = level_power(self.band, 40), 0

    # ---- control ----
    def open(self, cls, i):
        c = self.ch[cls][i]
        c.active = True
        if c.sacch:
            c.power, c.ta = level_power(self.band, 40), 0

    def close(self, cls, i):
        self.ch[cls][i].active = False

    def set_phy(self, i, power, ta):
        c = self.ch[XCCH][i]
        assert c.sacch and 0 <= power <= 40 and 0 <= ta <= 63
        c.power, c.ta = level_power(self.band, power), int(ta)

    # ---- calls ----
    walk = staticmethod(lmm.MuxModel.walk)

    def grid(self, fn, F):
        nb = [max([sum(1 for _, B in self.walk(c.m, fn, F) if B == 0) for c in self.ch[cls]], default=0) for cls in (TCH, XCCH)]
        return nb[0], nb[1], sum(len(self.walk(c.m, fn, F)) for c in self.ch[RACH])

    def encode(self, fn, F, tch_kind=None, tch_payload=None, xcch_kind=None, xcch_payload=None, rach_kind=None, rach_ra=None,
               rach_bsic=None, sib=None):
        """sib: dict of XCCH-indexed arrays power (dBm), ta (float32): the sibling L1Tx's current orders, or None."""
        A = self.comb.shape[0]
        bits = np.zeros((A, 8 * F, 148), np.uint8)
        what = np.zeros((A, 8 * F), np.uint8)
        who = np.full((A, 8 * F), -1, np.int32)
        if sib is not None:                                  # the call's snapshot
            for i, c in enumerate(self.ch[XCCH]):
                if c.sacch and c.active:
                    c.power = level_power(self.band, int(sib["power"][i]))
                    c.ta = int(np.float32(np.float32(sib["ta"][i]) + np.float32(0.5)))
        grids = {TCH: (tch_kind, tch_payload), XCCH: (xcch_kind, xcch_payload)}
        for cls in (TCH, XCCH):
            for i, c in enumerate(self.ch[cls]):
                b = 0
                for k, B in self.walk(c.m, fn, F):
                    if B == 0:
                        c.block = self._block(cls, i, c, b, grids[cls])
                        c.left = 4
                        b += 1
                    if c.block is not None and c.left == 4 - B:    # (a block begun before the object existed has no bursts)
                        s = 8 * k + c.tn
                        bits[c.a, s] = c.block[B]
                        what[c.a, s] = W_TCH if cls == TCH else W_XCCH
                        who[c.a, s] = i
                        c.left -= 1
        for c in self.ch[RACH]:
            for j, (k, _) in enumerate(self.walk(c.m, fn, F)):
                if rach_kind[j] == 1:
                    s = 8 * k + c.tn
                    bsic = self.bsic if rach_bsic is None else int(rach_bsic[j]) & 63
                    bits[c.a, s] = access_burst(self.o, int(rach_ra[j]), bsic)
                    what[c.a, s] = W_ACCESS
                    who[c.a, s] = j
        xc = self.ch[XCCH]
        return dict(bits=bits, what=what, who=who, ms_power=np.array([c.power for c in xc], np.int32),
                    ms_ta=np.array([c.ta for c in xc], np.int32),
                    tch_state=self.records(TCH), xcch_state=self.records(XCCH))

    def records(self, cls):
        chans = self.ch[cls]
        return np.stack([c.record() for c in chans]) if chans else np.zeros((0, STATE_BYTES), np.uint8)

    def _block(self, cls, i, c, b, grid):
        """The bursts of the channel's block b of the call, or None when nothing is sent."""
        if not c.active:
            return None
        kind, payload = grid
        if cls == TCH:
            tsc = [self.bsic & 7]
            blk, st = self.o.tch_encode_stream(np.array([[kind[i, b]]], np.uint8), payload[i, b].reshape(1, 1, 33), tsc,
                                               self.filler, c.tch_state.reshape(1, 32))
            blk = blk[0, 0]
            # c[] of the block: its even half rides in these bursts, its odd half in the next block's (read off a throw-away one)
            nxt, _ = self.o.tch_encode_stream(np.zeros((1, 1), np.uint8), np.zeros((1, 1, 33), np.uint8), tsc, self.filler,
                                              st[0].reshape(1, 32).copy())
            cc = np.where(_K % 8 < 4, blk[_K % 4, _E[_J]], nxt[0, 0][_K % 4, _E[_J]]).astype(np.uint8)
            c.tch_state = st[0]
            self._sent(c, cc, int(kind[i, b] == 2))
            return blk
        if kind[i, b] != 1:
            return None
        frame = np.array(payload[i, b], np.uint8)
        if c.sacch:
            frame[0], frame[1] = lmm.encode_power(self.band, c.power) & 31, c.ta
        blk = self.o.xcch_encode(frame, self.tsc).reshape(4, 148)
        self._sent(c, blk[_K % 4, _E[_J]].astype(np.uint8), 0)
        return blk

    @staticmethod
    def _sent(c, cc, facch):
        c.prev_c, c.prev_f = c.last_c, c.last_f
        c.last_c, c.last_f = cc, facch


# ---- what the tests of the model and of the device share: content that does not depend on how a span is cut into calls ----
class Content:
    """Payloads keyed by (class, channel, the block's first frame, unwrapped) and access bursts keyed by frame, so that any
    split of a span asks for the same.  speech: TCH blocks are speech or FACCH only, with the uncoded last four payload bits zero
    (what a decoder can give back)."""

    def __init__(self, rng, p_none=0.25, speech=False, p_wrong_bsic=0.3):
        self.rng, self.p_none, self.speech, self.p_wrong = rng, p_none, speech, p_wrong_bsic
        self.d = {}

    def get(self, cls, i, u):
        key = (cls, i, u)
        if key not in self.d:
            r = self.rng
            if cls == TCH:
                if self.speech:
                    kind = int(r.choice([1, 2], p=[0.7, 0.3]))
                    pl = r.integers(0, 256, 33).astype(np.uint8)
                    pl[32] &= 0xF0
                else:
                    kind = int(r.choice([0, 1, 1, 2, 3], p=[0.2, 0.35, 0.2, 0.2, 0.05]))
                    pl = r.integers(0, 256, 33).astype(np.uint8)
                self.d[key] = (kind, pl)
            elif cls == XCCH:
                self.d[key] = (0 if r.random() < self.p_none else 1, r.integers(0, 256, 23).astype(np.uint8))
            else:                                            # (kind, RA, BSIC or None for the cell's)
                self.d[key] = (0 if r.random() < self.p_none else 1, int(r.integers(0, 256)),
                               int(r.integers(0, 64)) if r.random() < self.p_wrong else None)
        return self.d[key]


def grids(model, content, fn, F):
    """The call's inputs from the model's walk of each channel: dict(tch_kind, tch_payload, xcch_kind, xcch_payload, rach_kind,
    rach_ra, rach_bsic), shaped by model.grid."""
    nbt, nbx, nr = model.grid(fn, F)
    out = {}
    for cls, key, nb, width in ((TCH, "tch", nbt, 33), (XCCH, "xcch", nbx, 23)):
        chans = model.ch[cls]
        kind = np.zeros((len(chans), nb), np.uint8)
        pay = np.zeros((len(chans), nb, width), np.uint8)
        for i, c in enumerate(chans):
            b = 0
            for k, B in model.walk(c.m, fn, F):
                if B == 0:
                    kind[i, b], pay[i, b] = content.get(cls, i, fn + k)
                    b += 1
        out[key + "_kind"], out[key + "_payload"] = kind, pay
    rk, ra, rb = np.zeros(nr, np.uint8), np.zeros(nr, np.uint8), np.full(nr, model.bsic, np.uint8)
    for c in model.ch[RACH]:
        for j, (k, _) in enumerate(model.walk(c.m, fn, F)):
            kind, v, bsic = content.get(RACH, 0, fn + k)
            rk[j], ra[j] = kind, v
            if bsic is not None:
                rb[j] = bsic
    out["rach_kind"], out["rach_ra"], out["rach_bsic"] = rk, ra, rb
    return out
