"""A literal model of the uplink L1 demultiplexer (trxsig_l1rx.h) on the CPU -- TEST INFRASTRUCTURE ONLY.

  ARFCNManager::installDecoder: mDemuxTable[TN][FN] for every FN + k * repeatLength < 5304, no entry written twice
  ARFCNManager::receiveBurst:   mDemuxTable[TN][FN % 5304], NULL drops the burst
  the wire parse:               RSSI = -(signed char)byte, timingError = int16 / 256.0F into an int
  XCCHL1Decoder / TCHFACCHL1Decoder::writeLowSide + processBurst: inactive ignores; B = reverseMapping(FN) % 4 / % 8
  RACHL1Decoder::writeLowSide:  tail bits, then the parity's BSIC against the cell's, then RA
  SACCHL1Decoder::handleGoodFrame / open: power = decodePower(mU.peekField(3,5)), TA = mU.peekField(9,7) if < 64; 40 / 0

The mappings come from tests/golden/tdma_uplink.npz (recorded from the reference's GSM/GSMTDMA.cpp), the decoders from
tests/fec_stream_model.py, whose Decoder is the reference's per-channel decoder driven one burst at a time.  Bursts are walked
in time order.  The outputs are laid out as the library lays them out: per class [n_chan][n_blocks], block b of a channel being
its b-th block whose closing (B % 4 == 3) frame is at or after the call's first frame."""
import os

import numpy as np

import fec_stream_model as fsm

MAX_MODULUS = 51 * 26 * 4
HYPERFRAME = 2048 * 26 * 51
TCH, XCCH, RACH = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tdma_uplink.npz")
POWER = {850: [39, 39, 39, 37, 35, 33, 31, 29, 27, 25, 23, 21, 19, 17, 15, 13, 11, 9, 7, 5] + [5] * 12,
         1800: [30, 28, 26, 24, 22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 0] + [0] * 13 + [36, 24, 23],
         1900: [30, 28, 26, 24, 22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 0] + [0] * 16}
POWER[900] = POWER[850]


class Mapping:
    def __init__(self, name, repeat, frames, allowed, c0only):
        self.name, self.R, self.frames = str(name), int(repeat), [int(f) for f in frames]
        self.allowed, self.c0only = int(allowed), bool(c0only)
        self.rev = [-1] * 104
        for i, f in enumerate(self.frames):
            self.rev[f] = i

    def reverse(self, fn):                                   # TDMAMapping::reverseMapping
        return self.rev[fn % self.R]


def load_mappings(path=GOLDEN):
    g = np.load(path)
    return {str(n): Mapping(n, r, fr[:k], al, c0) for n, r, fr, k, al, c0 in
            zip(g["names"], g["repeat"], g["frames"], g["nframes"], g["allowed"], g["c0only"])}


class Channel:
    def __init__(self, cls, a, tn, mapping, sub, prims):
        self.cls, self.a, self.tn, self.m, self.sub = cls, a, tn, mapping, sub
        self.sacch = mapping.name.startswith("SACCH")
        self.dec = fsm.Decoder(prims, cls == TCH) if cls != RACH else None
        self.active = True
        self.rssi = self.timing = 0
        self.power, self.ta = (40, 0) if self.sacch else (-1, -1)

    def open(self):                                           # L1Decoder::open (+ SACCHL1Decoder::open)
        self.active = True
        self.dec.fer = np.float32(0.0)
        if self.sacch:
            self.power, self.ta = 40, 0


def plan(comb, maps, prims):
    """The channels of a CMD SETSLOT plan comb[a][tn], per class, in the library's documented order."""
    ch = {TCH: [], XCCH: [], RACH: []}
    for a in range(comb.shape[0]):
        for tn in range(8):
            k = int(comb[a, tn])
            if k == 1:
                ch[TCH].append(Channel(TCH, a, tn, maps["FACCH_TCHF"], 0, prims))
                ch[XCCH].append(Channel(XCCH, a, tn, maps["SACCH_TF_T%d" % tn], 0, prims))
            elif k == 5:
                assert a == 0 and tn == 0
                ch[XCCH] += [Channel(XCCH, a, tn, maps["SDCCH_4_%dU" % s], s, prims) for s in range(4)]
                ch[XCCH] += [Channel(XCCH, a, tn, maps["SACCH_C4_%dU" % s], s, prims) for s in range(4)]
                ch[RACH].append(Channel(RACH, a, tn, maps["RACHC5"], 0, prims))
            elif k == 7:
                ch[XCCH] += [Channel(XCCH, a, tn, maps["SDCCH_8_%dU" % s], s, prims) for s in range(8)]
                ch[XCCH] += [Channel(XCCH, a, tn, maps["SACCH_C8_%dU" % s], s, prims) for s in range(8)]
            else:
                assert k == 0
    return ch


def install(chans, n_arfcn):
    """mDemuxTable per ARFCN, as installDecoder fills it: table[a][tn][FN] = channel (None: unconfigured)."""
    table = [[[None] * MAX_MODULUS for _ in range(8)] for _ in range(n_arfcn)]
    for cls in (TCH, XCCH, RACH):
        for c in chans[cls]:
            assert c.m.allowed >> c.tn & 1, (c.m.name, c.tn)
            for f in c.m.frames:
                fn = f
                while fn < MAX_MODULUS:
                    assert table[c.a][c.tn][fn] is None, (c.m.name, c.a, c.tn, fn)
                    table[c.a][c.tn][fn] = c
                    fn += c.m.R
    return table


def wire_phy(rssi, timing):
    """The datagram's RSSI byte and int16 timing, read back by TRXManager (TRXManager.cpp:220-233)."""
    r = int(np.int8(np.uint8(int(rssi) & 0xFF)))
    t = int(np.int16(np.uint16(int(timing) & 0xFFFF)))
    return -r, int(np.float32(t) / np.float32(256.0))         # float -> int: toward zero


class Model:
    def __init__(self, comb, bsic, band=900, prims=None):
        self.comb = np.asarray(comb, np.uint8)
        self.A = self.comb.shape[0]
        self.bsic, self.band = bsic, band
        self.p = prims or fsm.Prims()
        self.maps = load_mappings()
        self.ch = plan(self.comb, self.maps, self.p)
        self.table = install(self.ch, self.A)

    def next_closing(self, c, u):
        while c.m.reverse(u % HYPERFRAME) % 4 != 3 or c.m.reverse(u % HYPERFRAME) < 0:
            u += 1
        return u

    def closing_frames(self, c, fn, nb):
        """the frames (unwrapped, >= fn) of the channel's next nb closing bursts"""
        out, u = [], fn
        while len(out) < nb:
            r = c.m.reverse(u % HYPERFRAME)
            if r >= 0 and r % 4 == 3:
                out.append(u)
            u += 1
        return out

    def decode(self, col, fn, wire=True):
        """col: dict(valid[T, A], soft[T, A, 148], rssi[T, A], timing[T, A]) of whole frames from (fn, TN 0), as
        trxsig_trxgroup_collect returns them.  Returns the library's outputs (host arrays)."""
        valid, soft = np.asarray(col["valid"]), np.asarray(col["soft"], np.float32)
        F = valid.shape[0] // 8
        res = {c: {} for cls in (TCH, XCCH) for c in self.ch[cls]}     # channel -> {closing frame: (status, tch, l2, fer)}
        fer_log = {c: [(fn - 1, c.dec.fer)] for cls in (TCH, XCCH) for c in self.ch[cls]}
        rach = []
        for k in range(F):
            u = fn + k
            FN = u % HYPERFRAME
            for tn in range(8):
                for a in range(self.A):
                    if not valid[8 * k + tn, a]:
                        continue
                    c = self.table[a][tn][FN % MAX_MODULUS]        # receiveBurst
                    if c is None:
                        continue
                    v = soft[8 * k + tn, a, :148]
                    v = self.p.wire(v) if wire else v.copy()
                    rssi, timing = wire_phy(col["rssi"][8 * k + tn, a], col["timing"][8 * k + tn, a])
                    if c.cls == RACH:
                        r = self.p.fo.rach_decode(v[49:85])
                        ok = bool(r["tail_ok"]) and int(r["bsic"]) == self.bsic
                        rach.append((FN, a, rssi, timing, int(ok), int(r["ra"]) if ok else 0))
                        continue
                    if not c.active:
                        continue
                    c.rssi, c.timing = rssi, timing
                    B = c.m.reverse(FN) % (8 if c.cls == TCH else 4)
                    out = c.dec.burst(B, v)
                    if out is not None:
                        res[c][u] = out + (c.dec.fer,)
                        fer_log[c].append((u, c.dec.fer))
                        st, _, l2 = out
                        if c.sacch and st & fsm.TCH_GOOD:            # handleGoodFrame on the L2 frame bits (mD aliases mU)
                            bits = np.unpackbits(l2)
                            c.power = POWER[self.band][int("".join(map(str, bits[3:8])), 2)]
                            ta = int("".join(map(str, bits[9:16])), 2)
                            if ta < 64:
                                c.ta = ta
        out = {}
        for cls, key in ((TCH, "tch"), (XCCH, "xcch")):
            chans = self.ch[cls]
            nb = 0
            for c in chans:                                       # blocks with a burst position in the window
                blocks = {self.next_closing(c, u) for u in range(fn, fn + F) if c.m.reverse(u % HYPERFRAME) >= 0}
                nb = max(nb, len(blocks))
            S = len(chans)
            o = dict(status=np.zeros((S, nb), np.uint8), frames=np.zeros((S, nb, 33 if cls == TCH else 23), np.uint8),
                     facch=np.zeros((S, nb, 23), np.uint8), fer=np.zeros((S, nb), np.float32), fn=np.zeros((S, nb), np.int32),
                     state=np.stack([c.dec.state() for c in chans]) if S else np.zeros((0, 0), np.uint8),
                     rssi=np.array([c.rssi for c in chans], np.int32), timing=np.array([c.timing for c in chans], np.int32))
            for s, c in enumerate(chans):
                for b, f in enumerate(self.closing_frames(c, fn, nb)):
                    o["fn"][s, b] = f % HYPERFRAME
                    o["fer"][s, b] = [x for t, x in fer_log[c] if t <= f][-1]
                    if f in res[c]:
                        st, t33, l2, _ = res[c][f]
                        o["status"][s, b] = st
                        if cls == TCH:
                            o["frames"][s, b], o["facch"][s, b] = t33, l2
                        else:
                            o["frames"][s, b] = l2
            if cls == XCCH:
                o["power"] = np.array([c.power for c in chans], np.int32)
                o["ta"] = np.array([c.ta for c in chans], np.int32)
            out[key] = o
        out["rach"] = dict(fn=np.array([r[0] for r in rach], np.int32), arfcn=np.array([r[1] for r in rach], np.int32),
                           rssi=np.array([r[2] for r in rach], np.int32), timing=np.array([r[3] for r in rach], np.int32),
                           ok=np.array([r[4] for r in rach], np.uint8), ra=np.array([r[5] for r in rach], np.uint8))
        return out
