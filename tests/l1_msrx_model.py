"""A literal model of the mobile-side downlink L1 (trxsig_l1msrx.h) on the CPU -- TEST INFRASTRUCTURE ONLY.

Routing is a per-burst lookup, as a handset's (or ARFCNManager::receiveBurst's) demux table does it: TABLE[comb][TN][FN % 5304]
names the downlink mapping that owns the slot, built from tests/golden/tdma_downlink.npz (recorded from the reference's
GSM/GSMTDMA.cpp) by writing every mapping's frames + k * repeatLength below 5304.  Nothing here walks mapping positions.

  TCH / XCCH / CCCH / BCCH: tests/fec_stream_model.py's Decoder, the reference's per-channel decoder driven one burst at a time
                            (inactive ignores; B = reverseMapping(FN) % 8 or % 4); RSSI / timing through the wire parse
  SACCH orders:             SACCHL1Decoder::handleGoodFrame's reading of the L1 header: POWER[band][frame[0] & 31], frame[1] & 127
                            if below 64; 40 / 0 on a new object and on open
  BCCH:                     TC = (FN / 51) % 8 of the block's first burst
  SCH:                      OUR OWN decoder -- the reference only encodes SCH.  The inverse of SCHL1Encoder::generate from the
                            oracle's primitives: e = burst[3..42) + burst[106..145), FecOracle.viterbi_decode -> u[39], tail and
                            parity (generator 0x575, inverted), lsb8msb on the first three octets, BSIC(6) T1(11) T2(5) T3'(3)
  FCCH:                     the number of soft values above 0.5

Outputs are laid out as the library lays them out: per class [n_chan][n_blocks], block b of a channel being its b-th block whose
closing (B % 4 == 3) frame is at or after the call's first frame; XCCH, CCCH and BCCH share one grid width."""
import os

import numpy as np

import fec_stream_model as fsm

MAX_MODULUS = 51 * 26 * 4
HYPERFRAME = 2048 * 26 * 51
TCH, XCCH, CCCH, BCCH, SCH, FCCH = 0, 1, 3, 4, 5, 6
BLOCK_CLASSES = (TCH, XCCH, CCCH, BCCH)
KEYS = {TCH: "tch", XCCH: "xcch", CCCH: "ccch", BCCH: "bcch"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tdma_downlink.npz")
POWER = {850: [39, 39, 39, 37, 35, 33, 31, 29, 27, 25, 23, 21, 19, 17, 15, 13, 11, 9, 7, 5] + [5] * 12,
         1800: [30, 28, 26, 24, 22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 0] + [0] * 13 + [36, 24, 23],
         1900: [30, 28, 26, 24, 22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 0] + [0] * 16}
POWER[900] = POWER[850]
SCH_POLY = 0x575


class Mapping:
    def __init__(self, name, repeat, frames):
        self.name, self.R, self.frames = str(name), int(repeat), [int(f) for f in frames]
        self.rev = [-1] * 104
        for i, f in enumerate(self.frames):
            self.rev[f] = i

    def reverse(self, fn):                                   # TDMAMapping::reverseMapping
        return self.rev[fn % self.R]


def load_mappings(path=GOLDEN):
    g = np.load(path)
    return {str(n): Mapping(n, r, fr[:k]) for n, r, fr, k in zip(g["names"], g["repeat"], g["frames"], g["nframes"])}


def slot_mappings(comb, tn):
    """the names of the downlink mappings that share a slot of combination comb on timeslot tn"""
    if comb == 1:
        return ["FACCH_TCHF", "SACCH_TF_T%d" % tn]
    if comb == 5:
        return ["SDCCH_4_%dD" % s for s in range(4)] + ["SACCH_C4_%dD" % s for s in range(4)] + \
               ["CCCH_%d" % s for s in range(3)] + ["BCCH", "SCH", "FCCH"]
    if comb == 7:
        return ["SDCCH_8_%dD" % s for s in range(8)] + ["SACCH_C8_%dD" % s for s in range(8)]
    raise ValueError("unsupported combination %r" % comb)


def slot_table(maps, comb, tn):
    """(table[FN % 5304] -> mapping name or None, [(fn, first, second)] collisions) of one slot"""
    table, clash = [None] * MAX_MODULUS, []
    for name in slot_mappings(comb, tn):
        m = maps[name]
        for f in m.frames:
            for fn in range(f, MAX_MODULUS, m.R):
                if table[fn] is not None:
                    clash.append((fn, table[fn], name))
                table[fn] = name
    return table, clash


class Channel:
    def __init__(self, cls, a, tn, mapping, sub, prims):
        self.cls, self.a, self.tn, self.m, self.sub = cls, a, tn, mapping, sub
        self.sacch = mapping.name.startswith("SACCH")
        self.dec = fsm.Decoder(prims, cls == TCH) if cls in BLOCK_CLASSES else None
        self.active = True
        self.rssi = self.timing = 0
        self.power, self.ta = (40, 0) if self.sacch else (-1, -1)

    def open(self):
        self.active = True
        self.dec.fer = np.float32(0.0)
        if self.sacch:
            self.power, self.ta = 40, 0


def wire_phy(rssi, timing):
    """The datagram's RSSI byte and int16 timing, read back as TRXManager reads them (tests/l1_demux_model.py)."""
    r = int(np.int8(np.uint8(int(rssi) & 0xFF)))
    t = int(np.int16(np.uint16(int(timing) & 0xFFFF)))
    return -r, int(np.float32(t) / np.float32(256.0))


def field(bits, at, n):
    v = 0
    for b in bits[at:at + n]:
        v = (v << 1) | int(b)
    return v


def sch_decode(fo, v):
    """v: the burst's 148 soft values as the decoder sees them -> (ok, bsic, rfn)"""
    e = np.concatenate([v[3:42], v[106:145]]).astype(np.float32)
    u = fo.viterbi_decode(e, 39)
    par = (~fo.parity(SCH_POLY, 10, u[:25])) & 0x3FF
    ok = not u[35:39].any() and field(u, 25, 10) == par
    d = u[:25].copy()
    d[:24] = fo.lsb8msb(d[:24])
    bsic, t1, t2, t3p = field(d, 0, 6), field(d, 6, 11), field(d, 17, 5), field(d, 22, 3)
    t3 = 10 * t3p + 1
    return bool(ok), bsic, 1326 * t1 + 51 * ((t3 - t2) % 26) + t3


class Model:
    def __init__(self, comb, bsic, band=900, prims=None, maps=None):
        self.comb = np.asarray(comb, np.uint8)
        self.A = self.comb.shape[0]
        self.bsic, self.band = int(bsic), int(band)
        self.p = prims or fsm.Prims()
        self.maps = M = maps or load_mappings()
        self.ch = {c: [] for c in (TCH, XCCH, CCCH, BCCH, SCH, FCCH)}
        self.tables, self.by_name = {}, {}
        for a in range(self.A):
            for tn in range(8):
                k = int(self.comb[a, tn])
                if k == 0:
                    continue
                if k == 5:
                    assert a == 0 and tn == 0
                self.tables[(a, tn)], clash = slot_table(M, k, tn)
                assert not clash, clash
                new = []
                for name in slot_mappings(k, tn):
                    cls = TCH if name == "FACCH_TCHF" else CCCH if name.startswith("CCCH") else BCCH if name == "BCCH" else \
                        SCH if name == "SCH" else FCCH if name == "FCCH" else XCCH
                    sub = int(name.split("_")[2][0]) if name[:5] in ("SDCCH", "SACCH") and not name.startswith("SACCH_TF") else \
                        int(name[-1]) if cls == CCCH else 0
                    new.append(Channel(cls, a, tn, M[name], sub, self.p))
                for c in new:
                    self.ch[c.cls].append(c)
                    self.by_name[(a, tn, c.m.name)] = c

    def route(self, a, tn, FN):
        """the channel that owns (ARFCN, TN, FN), or None"""
        t = self.tables.get((a, tn))
        name = t[FN % MAX_MODULUS] if t is not None else None
        return self.by_name[(a, tn, name)] if name is not None else None

    def next_closing(self, c, u):
        while c.m.reverse(u % HYPERFRAME) < 0 or c.m.reverse(u % HYPERFRAME) % 4 != 3:
            u += 1
        return u

    def closing_frames(self, c, fn, nb):
        out, u = [], fn
        while len(out) < nb:
            r = c.m.reverse(u % HYPERFRAME)
            if r >= 0 and r % 4 == 3:
                out.append(u)
            u += 1
        return out

    def first_frame(self, c, closing):
        u = closing
        while c.m.reverse(u % HYPERFRAME) % 4 != 0:
            u -= 1
            while c.m.reverse(u % HYPERFRAME) < 0:
                u -= 1
        return u

    def decode(self, col, fn, wire=True):
        """col: dict(valid[T, A], soft[T, A, 148], rssi[T, A], timing[T, A]) of whole frames from (fn, TN 0), as
        trxsig_trxgroup_collect returns them.  Returns the library's outputs (host arrays)."""
        valid, soft = np.asarray(col["valid"]), np.asarray(col["soft"], np.float32)
        F = valid.shape[0] // 8
        blockch = [c for cls in BLOCK_CLASSES for c in self.ch[cls]]
        res = {c: {} for c in blockch}
        fer_log = {c: [(fn - 1, c.dec.fer)] for c in blockch}
        sch = dict(fn=[], present=[], ok=[], bsic=[], rfn=[], sync=[])
        fcch = dict(fn=[], ones=[])
        for k in range(F):
            u = fn + k
            FN = u % HYPERFRAME
            for tn in range(8):
                for a in range(self.A):
                    c = self.route(a, tn, FN)
                    if c is None:
                        continue
                    here = bool(valid[8 * k + tn, a])
                    v = None
                    if here:
                        v = soft[8 * k + tn, a, :148]
                        v = self.p.wire(v) if wire else v.copy()
                    if c.cls == SCH:
                        ok, bsic, rfn = sch_decode(self.p.fo, v) if here else (False, 0, 0)
                        for key, val in (("fn", FN), ("present", here), ("ok", ok), ("bsic", bsic), ("rfn", rfn),
                                         ("sync", ok and rfn == FN and bsic == self.bsic)):
                            sch[key].append(int(val))
                        continue
                    if c.cls == FCCH:
                        fcch["fn"].append(FN)
                        fcch["ones"].append(int((v > np.float32(0.5)).sum()) if here else -1)
                        continue
                    if not here or not c.active:
                        continue
                    c.rssi, c.timing = wire_phy(col["rssi"][8 * k + tn, a], col["timing"][8 * k + tn, a])
                    B = c.m.reverse(FN) % (8 if c.cls == TCH else 4)
                    out = c.dec.burst(B, v)
                    if out is not None:
                        res[c][u] = out
                        fer_log[c].append((u, c.dec.fer))
                        st, _, l2 = out
                        if c.sacch and st & fsm.TCH_GOOD:
                            c.power = POWER[self.band][int(l2[0]) & 31]
                            if int(l2[1]) & 127 < 64:
                                c.ta = int(l2[1]) & 127
        out = {}

        def n_blocks(chans):
            nb = 0
            for c in chans:
                blocks = {self.next_closing(c, u) for u in range(fn, fn + F) if c.m.reverse(u % HYPERFRAME) >= 0}
                nb = max(nb, len(blocks))
            return nb
        nb_ctl = n_blocks([c for cls in (XCCH, CCCH, BCCH) for c in self.ch[cls]])
        for cls in BLOCK_CLASSES:
            chans = self.ch[cls]
            nb = n_blocks(chans) if cls == TCH else nb_ctl
            S = len(chans)
            nbytes = fsm.TCH_STATE_BYTES if cls == TCH else fsm.XCCH_STATE_BYTES
            o = dict(status=np.zeros((S, nb), np.uint8), frames=np.zeros((S, nb, 33 if cls == TCH else 23), np.uint8),
                     facch=np.zeros((S, nb, 23), np.uint8), fer=np.zeros((S, nb), np.float32), fn=np.zeros((S, nb), np.int32),
                     tc=np.zeros((S, nb), np.int32),
                     state=np.stack([c.dec.state() for c in chans]) if S else np.zeros((0, nbytes), np.uint8),
                     rssi=np.array([c.rssi for c in chans], np.int32), timing=np.array([c.timing for c in chans], np.int32))
            for s, c in enumerate(chans):
                for b, f in enumerate(self.closing_frames(c, fn, nb)):
                    o["fn"][s, b] = f % HYPERFRAME
                    o["fer"][s, b] = [x for t, x in fer_log[c] if t <= f][-1]
                    if cls == BCCH:
                        o["tc"][s, b] = ((self.first_frame(c, f) % HYPERFRAME) // 51) % 8
                    if f in res[c]:
                        st, t33, l2 = res[c][f]
                        o["status"][s, b] = st
                        if cls == TCH:
                            o["frames"][s, b], o["facch"][s, b] = t33, l2
                        else:
                            o["frames"][s, b] = l2
            if cls == XCCH:
                o["power"] = np.array([c.power for c in chans], np.int32)
                o["ta"] = np.array([c.ta for c in chans], np.int32)
            out[KEYS[cls]] = o
        out["sch"] = {k: np.array(v, np.int32 if k in ("fn", "rfn") else np.uint8) for k, v in sch.items()}
        out["fcch"] = {k: np.array(v, np.int32) for k, v in fcch.items()}
        return out


# ---- helpers shared by the CPU and GPU tests ----
def col_from_bits(rng, bits, what=None, noise=0.3):
    """A downlink encode's bits [A][8 F][148] (trxsig_l1tx's d_bits, or tests/l1_mux_model.py's) as the model's input: every slot
    present (only the non-empty ones where `what` is given), soft values fec_stream_model.soft_from_bits, RSSI / timing 0."""
    bits = np.asarray(bits, np.uint8)
    A, T, _ = bits.shape
    soft = fsm.soft_from_bits(rng, bits.transpose(1, 0, 2), noise)
    valid = np.ones((T, A), bool) if what is None else (np.asarray(what).T != 0)
    return dict(valid=valid, soft=soft, rssi=np.zeros((T, A), np.int64), timing=np.zeros((T, A), np.int64))


def cut(col, lo, hi):
    """frames [lo, hi) of a model input"""
    return {k: v[8 * lo:8 * hi] for k, v in col.items()}


def blocks_by_fn(out):
    """the decoded blocks of a model / library output, keyed by (class key, channel, closing FN)"""
    got = {}
    for key in ("tch", "xcch", "ccch", "bcch"):
        o = out[key]
        for s, b in zip(*np.nonzero(o["status"])):
            got[(key, int(s), int(o["fn"][s, b]))] = (int(o["status"][s, b]), o["frames"][s, b].tobytes(), o["facch"][s, b].tobytes(),
                                                      np.float32(o["fer"][s, b]).tobytes(), int(o["tc"][s, b]))
    return got
