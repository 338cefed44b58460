"""A literal model of the downlink L1 multiplexer (trxsig_l1tx.h) on the CPU -- TEST INFRASTRUCTURE ONLY.

  L1Encoder::rollForward:       each encoder walks its downlink TDMAMapping frame by frame (Time::rollForward: the next FN whose
                                FN % repeatLength is frameMapping(mTotalBursts)); a burst's B is reverseMapping(FN) % 4, a block
                                starts at B == 0 (on GSM 05.02's block grid, trxsig_l1tx.h's stated deviation)
  XCCHL1Encoder::sendFrame:     the oracle's fo_xcch_encode (LSB8MSB, Fire parity, coder, 4.1.4 interleave, TSC = BCC)
  SACCHL1Encoder::sendFrame:    phyNew from the sibling's accepted-burst counter, the float32 orders as written, mU.fillField of
                                the header before the frame is copied in at bit 16, then the XCCH encoder
  TCHFACCHL1Encoder::dispatch:  the oracle's fo_tch_encode_stream, its 32-byte state chained block to block
  BCCHL1Encoder::generate:      TC = (FN / 51) % 8 -> SI1, 2, 3, 4, 3, 2, 3, 4
  SCHL1Encoder::generate:       the oracle's fo_sch_encode for the burst's own FN; FCCH: 148 zeros
  L1Encoder::close / sendIdleFill: the next numFrames positions after the pending bursts carry the dummy burst

The mappings come from tests/golden/tdma_downlink.npz (recorded from the reference's GSM/GSMTDMA.cpp).  Outputs are laid out as
the library lays them out: bits [n_arfcn][8 F][148], what [n_arfcn][8 F], orders per XCCH channel."""
import math
import os

import numpy as np

import fectxbind

HYPERFRAME = 2048 * 26 * 51
TCH, XCCH, RACH, CCCH, BCCH = 0, 1, 2, 3, 4
W_NONE, W_FCCH, W_SCH, W_BCCH, W_CCCH, W_XCCH, W_TCH, W_IDLE = range(8)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tdma_downlink.npz")
DUMMY = np.array([int(ch) for ch in "0001111101101110110000010100100111000001001000100000001111100011100010111000101110001010111010010100"
                  "011001100111001111010011111000100101111101010000"], np.uint8)
POWER = {850: [39, 39, 39, 37, 35, 33, 31, 29, 27, 25, 23, 21, 19, 17, 15, 13, 11, 9, 7, 5] + [5] * 12,
         1800: [30, 28, 26, 24, 22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 0] + [0] * 13 + [36, 24, 23],
         1900: [30, 28, 26, 24, 22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 0] + [0] * 16}
POWER[900] = POWER[850]
SI_OF_TC = [0, 1, 2, 3, 2, 1, 2, 3]


class Mapping:
    def __init__(self, name, repeat, frames):
        self.name, self.R, self.frames = str(name), int(repeat), [int(f) for f in frames]
        self.n = len(self.frames)
        self.rev = [-1] * 104
        for i, f in enumerate(self.frames):
            self.rev[f] = i

    def reverse(self, fn):                                   # TDMAMapping::reverseMapping
        return self.rev[fn % self.R]


def load_mappings(path=GOLDEN):
    g = np.load(path)
    return {str(n): Mapping(n, r, fr[:k]) for n, r, fr, k in zip(g["names"], g["repeat"], g["frames"], g["nframes"])}


def roll_forward(fn, wfn, modulus):
    """Time::rollForward (GSMCommon.h:342-346)"""
    while fn % modulus != wfn:
        fn = (fn + 1) % HYPERFRAME
    return fn


def c_round(x):
    """C's round(): halfway cases away from zero"""
    x = float(x)
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def encode_power(band, power):
    """encodePower (GSML1FEC.cpp:146-173)"""
    table = POWER[band]
    min_err, code = abs(power - table[0]), 0
    for i in range(1, 32):
        e = abs(power - table[i])
        if e == 0:
            return i
        if e < min_err:
            min_err, code = e, i
    return code


def sacch_orders(rssi, target, actual_power, actual_ta, timing_error):
    """SACCHL1Encoder::sendFrame's phyNew branch in float32 as written -> (ordered power (int), ordered TA (float32))"""
    f32 = np.float32
    delta = f32(f32(rssi) - f32(target))
    p = int(f32(f32(actual_power) - f32(c_round(f32(delta * f32(0.5))))))
    p = 40 if p > 40 else 0 if p < 0 else p
    t = f32(f32(actual_ta) - f32(f32(0.5) * f32(timing_error)))
    if t > f32(63.0):
        t = f32(63.0)
    if t < f32(0.0):
        t = f32(0.0)
    return p, t


def sacch_header(band, power, ta):
    """mU.fillField(0, encodePower(power), 8); mU.fillField(8, (int)(ta + 0.5F), 8) -> the two header octets"""
    return encode_power(band, power) & 0xff, int(np.float32(ta + np.float32(0.5))) & 0xff


class Channel:
    def __init__(self, cls, a, tn, mapping, sub):
        self.cls, self.a, self.tn, self.m, self.sub = cls, a, tn, mapping, sub
        self.sacch = mapping.name.startswith("SACCH")
        self.active = True
        self.block = None                                    # bursts [4][148] of the block being sent, or None
        self.tch_state = np.zeros(32, np.uint8)
        self.idle_left = 0
        self.power, self.ta = (40, np.float32(0.0)) if self.sacch else (-1, np.float32(-1.0))
        self.seen = 0


class MuxModel:
    def __init__(self, comb, bsic, band=900, rssi_target=-15.0, oracle=None, maps=None):
        self.comb = np.asarray(comb, np.uint8)
        self.bsic, self.band, self.target = int(bsic), int(band), float(rssi_target)
        self.o = oracle or fectxbind.FecTxOracle()
        self.maps = maps or load_mappings()
        self.tsc = fectxbind.TSC_BITS[self.bsic & 7]
        self.filler = np.zeros(456, np.uint8)
        self.si = None
        M = self.maps
        self.ch = {TCH: [], XCCH: [], CCCH: [], BCCH: []}
        self.gen = []                                        # (arfcn, tn, mapping, code) of FCCH / SCH
        for a in range(self.comb.shape[0]):
            for tn in range(8):
                k = int(self.comb[a, tn])
                if k == 1:
                    self.ch[TCH].append(Channel(TCH, a, tn, M["FACCH_TCHF"], 0))
                    self.ch[XCCH].append(Channel(XCCH, a, tn, M["SACCH_TF_T%d" % tn], 0))
                elif k == 5:
                    self.ch[XCCH] += [Channel(XCCH, a, tn, M["SDCCH_4_%dD" % s], s) for s in range(4)]
                    self.ch[XCCH] += [Channel(XCCH, a, tn, M["SACCH_C4_%dD" % s], s) for s in range(4)]
                    self.ch[CCCH] += [Channel(CCCH, a, tn, M["CCCH_%d" % s], s) for s in range(3)]
                    self.ch[BCCH].append(Channel(BCCH, a, tn, M["BCCH"], 0))
                    self.gen += [(a, tn, M["FCCH"], W_FCCH), (a, tn, M["SCH"], W_SCH)]
                elif k == 7:
                    self.ch[XCCH] += [Channel(XCCH, a, tn, M["SDCCH_8_%dD" % s], s) for s in range(8)]
                    self.ch[XCCH] += [Channel(XCCH, a, tn, M["SACCH_C8_%dD" % s], s) for s in range(8)]
                elif k != 0:
                    raise ValueError("unsupported combination")

    # ---- control ----
    def open(self, cls, i):                                  # L1Encoder::open (+ SACCHL1Encoder::open); idle fill cancelled
        c = self.ch[cls][i]
        c.active = True
        c.idle_left = 0
        if c.sacch:
            c.power, c.ta = 40, np.float32(0.0)

    def close(self, cls, i):                                 # L1Encoder::close -> sendIdleFill
        c = self.ch[cls][i]
        c.active = False
        c.idle_left = c.m.n

    def set_si(self, si):
        self.si = np.array(si, np.uint8).reshape(4, 23)

    # ---- walk ----
    @staticmethod
    def walk(m, fn, F):
        """The mapping's bursts in frames [fn, fn + F) (unwrapped), in time order: (k = frame - fn, B).  mNextWriteTime starts at
        the first frame at or after fn that carries the mapping (resync), then L1Encoder::rollForward: mTotalBursts + 1 and
        Time::rollForward to frameMapping(mTotalBursts) (repeatLength divides the hyperframe, so unwrapped frames walk alike)."""
        out = []
        u = fn
        while m.reverse(u) < 0:
            u += 1
        total = m.reverse(u)
        while u < fn + F:
            out.append((u - fn, total % 4))
            total = (total + 1) % m.n
            while u % m.R != m.frames[total]:
                u += 1
        return out

    def grid(self, fn, F):
        nb = {}
        for cls in (TCH, XCCH, CCCH):
            nb[cls] = max([sum(1 for _, B in self.walk(c.m, fn, F) if B == 0) for c in self.ch[cls]], default=0)
        return nb[TCH], nb[XCCH], nb[CCCH]

    def encode(self, fn, F, tch_kind=None, tch_payload=None, xcch_kind=None, xcch_payload=None, ccch_kind=None,
               ccch_payload=None, sib=None):
        """sib: dict of XCCH-indexed arrays rssi, timing, power, ta, count (the sibling L1Rx's state), or None."""
        A = self.comb.shape[0]
        bits = np.zeros((A, 8 * F, 148), np.uint8)
        what = np.zeros((A, 8 * F), np.uint8)
        for a, tn, m, code in self.gen:
            for k, _ in self.walk(m, fn, F):
                what[a, 8 * k + tn] = code
                if code == W_SCH:
                    bits[a, 8 * k + tn] = self.o.sch_encode([(fn + k) % HYPERFRAME], [self.bsic])[0]
        grids = {TCH: (tch_kind, tch_payload), XCCH: (xcch_kind, xcch_payload), CCCH: (ccch_kind, ccch_payload)}
        code_of = {TCH: W_TCH, XCCH: W_XCCH, CCCH: W_CCCH, BCCH: W_BCCH}
        for cls in (TCH, XCCH, CCCH, BCCH):
            for i, c in enumerate(self.ch[cls]):
                b = 0
                for k, B in self.walk(c.m, fn, F):
                    if B == 0:
                        c.block = self._block(cls, i, c, b, fn + k, grids.get(cls), sib)
                        b += 1
                    s = 8 * k + c.tn
                    if c.block is not None:
                        bits[c.a, s] = c.block[B]
                        what[c.a, s] = code_of[cls]
                    elif c.idle_left > 0:                    # sendIdleFill: after the pending bursts
                        bits[c.a, s] = DUMMY
                        what[c.a, s] = W_IDLE
                        c.idle_left -= 1
        xc = self.ch[XCCH]
        return dict(bits=bits, what=what, ms_power=np.array([c.power for c in xc], np.int32),
                    ms_ta=np.array([c.ta for c in xc], np.float32))

    def _block(self, cls, i, c, b, u, grid, sib):
        """The bursts of the channel's block b starting at frame u (unwrapped), or None when nothing is sent."""
        if cls == BCCH:
            if self.si is None:
                return None
            tc = ((u % HYPERFRAME) // 51) % 8
            return self.o.xcch_encode(self.si[SI_OF_TC[tc]], self.tsc)
        if not c.active:
            return None
        kind, payload = grid
        if cls == TCH:
            bits, st = self.o.tch_encode_stream(np.array([[kind[i, b]]], np.uint8), payload[i, b].reshape(1, 1, 33),
                                                [self.tsc_index()], self.filler, c.tch_state.reshape(1, 32))
            c.tch_state = st[0]
            return bits[0, 0]
        if kind[i, b] != 1:
            return None
        frame = np.array(payload[i, b], np.uint8)
        if c.sacch:
            if sib is not None and int(sib["count"][i]) != c.seen:     # phyNew: consumed by this (the call's first) block
                c.power, c.ta = sacch_orders(sib["rssi"][i], self.target, sib["power"][i], sib["ta"][i], sib["timing"][i])
                c.seen = int(sib["count"][i])
            frame = self.sacch_frame(frame, c.power, c.ta)
        return self.o.xcch_encode(frame, self.tsc)

    def tsc_index(self):
        return self.bsic & 7

    def sacch_frame(self, frame23, power, ta):
        """The 23 octets XCCHL1Encoder::sendFrame codes for a SACCH frame: the header in octets 0..1, the L2 frame's 21 octets
        (octets 2..22 of the caller's frame) after it"""
        h0, h1 = sacch_header(self.band, power, ta)
        f = np.array(frame23, np.uint8).copy()
        f[0], f[1] = h0, h1
        return f
