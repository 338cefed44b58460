"""A literal model of the ciphering stage (trxsig_l1ciph.h) on the CPU -- TEST INFRASTRUCTURE ONLY.  Pure Python and numpy.

  A5/1 (GSM 03.20 Annex C):  three shift registers, R = ((R << 1) & mask) | feedback per clock
                               R1 19 bits, feedback 18 ^ 17 ^ 16 ^ 13, clocking bit 8,  output bit 18
                               R2 22 bits, feedback 21 ^ 20,           clocking bit 10, output bit 21
                               R3 23 bits, feedback 22 ^ 21 ^ 20 ^ 7,  clocking bit 10, output bit 22
                             key: 64 clocks of all three, key bit (kc[i / 8] >> (i & 7)) & 1 into bit 0 after each; then 22 with
                             (count >> i) & 1; 100 majority-clocked steps thrown away; 228 more, one output bit after each:
                             BLOCK1 = the first 114 (downlink), BLOCK2 = the next 114 (uplink)
  COUNT:                     (T1 << 11) | (T3 << 5) | T2, T1 = FN / 1326, T3 = FN % 51, T2 = FN % 26
  where it lands:            keystream bit k at burst bit 3 + k (k < 57) or 31 + k: the payload bits 3..59 and 88..144
  routing:                   slot (a, t) of a call from fn has FN = (fn + t / 8) % 2715648 and TN = t % 8; it belongs to the TCH or
                             XCCH channel whose mapping (the tables the encoders' models walk: tests/golden/tdma_downlink.npz,
                             tdma_uplink.npz) holds FN on that (ARFCN, TN), or to none

`a5_1` is the statement word for word on Python integers; `keystream` is the same on numpy arrays, a slot per element, and is
what the operations use (tests/test_l1_ciph_model.py holds the two equal)."""
import numpy as np

import l1_ms_model as lms
import l1_mux_model as lmm

HYPERFRAME = 2048 * 26 * 51
TCH, XCCH = 0, 1
A5_1 = 1
M1, M2, M3 = (1 << 19) - 1, (1 << 22) - 1, (1 << 23) - 1
POS = np.r_[3:60, 88:145]                                   # burst bit of keystream bit k


def _fb(r1, r2, r3):
    return (((r1 >> 18) ^ (r1 >> 17) ^ (r1 >> 16) ^ (r1 >> 13)) & 1, ((r2 >> 21) ^ (r2 >> 20)) & 1,
            ((r3 >> 22) ^ (r3 >> 21) ^ (r3 >> 20) ^ (r3 >> 7)) & 1)


def _clock_all(r, bit):
    f = _fb(*r)
    return ((((r[0] << 1) & M1) | f[0]) ^ bit, (((r[1] << 1) & M2) | f[1]) ^ bit, (((r[2] << 1) & M3) | f[2]) ^ bit)


def _clock_maj(r):
    """one majority-clocked step (numpy arrays or ints)"""
    c = ((r[0] >> 8) & 1, (r[1] >> 10) & 1, (r[2] >> 10) & 1)
    m = (c[0] & c[1]) | (c[0] & c[2]) | (c[1] & c[2])
    f = _fb(*r)
    n = (((r[0] << 1) & M1) | f[0], ((r[1] << 1) & M2) | f[1], ((r[2] << 1) & M3) | f[2])
    if isinstance(m, np.ndarray):
        return tuple(np.where(c[i] == m, n[i], r[i]) for i in range(3))
    return tuple(n[i] if c[i] == m else r[i] for i in range(3))


def key_registers(kc):
    """(R1, R2, R3) after the 64 key steps"""
    r = (0, 0, 0)
    for i in range(64):
        r = _clock_all(r, (int(kc[i // 8]) >> (i & 7)) & 1)
    return r


def a5_1(kc, count):
    """(BLOCK1, BLOCK2): uint8 [114] each, one bit per byte"""
    r = key_registers(kc)
    for i in range(22):
        r = _clock_all(r, (int(count) >> i) & 1)
    for _ in range(100):
        r = _clock_maj(r)
    out = np.zeros(228, np.uint8)
    for k in range(228):
        r = _clock_maj(r)
        out[k] = ((r[0] >> 18) ^ (r[1] >> 21) ^ (r[2] >> 22)) & 1
    return out[:114], out[114:]


def keystream(regs, count):
    """regs: uint32 [n][3] after the key; count: [n] -> (BLOCK1, BLOCK2) uint8 [n][114] each"""
    regs = np.asarray(regs, np.uint32).reshape(-1, 3)
    count = np.asarray(count, np.uint32).reshape(-1)
    r = (regs[:, 0].copy(), regs[:, 1].copy(), regs[:, 2].copy())
    for i in range(22):
        r = _clock_all(r, (count >> np.uint32(i)) & np.uint32(1))
    for _ in range(100):
        r = _clock_maj(r)
    out = np.zeros((len(count), 228), np.uint8)
    for k in range(228):
        r = _clock_maj(r)
        out[:, k] = ((r[0] >> 18) ^ (r[1] >> 21) ^ (r[2] >> 22)) & 1
    return out[:, :114], out[:, 114:]


def blocks_batch(kc, count):
    """the primitive: kc uint8 [n][8], count [n] -> (BLOCK1, BLOCK2) [n][114]"""
    kc = np.asarray(kc, np.uint8).reshape(-1, 8)
    return keystream(np.array([key_registers(k) for k in kc], np.uint32).reshape(-1, 3), count)


def count_of(fn):
    fn = np.asarray(fn, np.int64)
    return (((fn // 1326) << 11) | ((fn % 51) << 5) | (fn % 26)).astype(np.uint32)


class CiphModel:
    """The object: the plan's TCH and XCCH channels (numbered as every L1 object numbers them), a key per channel."""

    def __init__(self, comb, maps_dl=None, maps_ul=None):
        self.comb = np.asarray(comb, np.uint8)
        dl, ul = maps_dl or lmm.load_mappings(), maps_ul or lms.load_mappings()
        self.ch = {TCH: [], XCCH: []}                       # (arfcn, tn, downlink mapping, uplink mapping)
        for a in range(self.comb.shape[0]):
            for tn in range(8):
                k = int(self.comb[a, tn])
                if k == 1:
                    self.ch[TCH].append((a, tn, dl["FACCH_TCHF"], ul["FACCH_TCHF"]))
                    self.ch[XCCH].append((a, tn, dl["SACCH_TF_T%d" % tn], ul["SACCH_TF_T%d" % tn]))
                elif k in (5, 7):
                    if k == 5 and (a, tn) != (0, 0):
                        raise ValueError("combination V on TN 0 of ARFCN 0 only")
                    n, tag = (4, "4") if k == 5 else (8, "8")
                    for name in ("SDCCH_%s_%d", "SACCH_C%s_%d"):
                        self.ch[XCCH] += [(a, tn, dl[(name + "D") % (tag, s)], ul[(name + "U") % (tag, s)]) for s in range(n)]
                elif k != 0:
                    raise ValueError("unsupported combination")
        self.algo = {c: np.zeros(len(self.ch[c]), np.uint32) for c in (TCH, XCCH)}
        self.regs = {c: np.zeros((len(self.ch[c]), 3), np.uint32) for c in (TCH, XCCH)}

    def set(self, cls, chan, algo, kc=None):
        assert algo in (0, A5_1) and 0 <= chan < len(self.ch[cls])
        self.algo[cls][chan] = algo
        self.regs[cls][chan] = key_registers(kc) if algo else (0, 0, 0)

    def state(self, cls):
        """the device records: uint32 [n_chan][4] = algo, R1, R2, R3"""
        return np.concatenate([self.algo[cls][:, None], self.regs[cls]], axis=1).astype(np.uint32)

    def route(self, uplink, fn, F):
        """(cls, chan) int32 [A][8 F], -1 where the slot belongs to no TCH or XCCH channel"""
        A = self.comb.shape[0]
        cls = np.full((A, 8 * F), -1, np.int32)
        chan = np.full((A, 8 * F), -1, np.int32)
        FN = (fn + np.arange(F)) % HYPERFRAME
        for c in (TCH, XCCH):
            for i, (a, tn, mdl, mul) in enumerate(self.ch[c]):
                m = mul if uplink else mdl
                on = np.array([m.reverse(int(u)) >= 0 for u in FN])
                assert (cls[a, tn::8][on] < 0).all(), "two mappings on one slot"
                cls[a, tn::8][on] = c
                chan[a, tn::8][on] = i
        return cls, chan

    def slot_keystream(self, uplink, fn, F, eligible=None):
        """(on [A][8 F] bool, ks [A][8 F][114] uint8: zero where not on)"""
        cls, chan = self.route(uplink, fn, F)
        on = np.zeros(cls.shape, bool)
        regs = np.zeros(cls.shape + (3,), np.uint32)
        for c in (TCH, XCCH):
            sel = cls == c
            on[sel] = self.algo[c][chan[sel]] != 0
            regs[sel] = self.regs[c][chan[sel]]
        if eligible is not None:
            on &= eligible
        ks = np.zeros(cls.shape + (114,), np.uint8)
        if on.any():
            FN = np.broadcast_to(np.repeat((fn + np.arange(F)) % HYPERFRAME, 8), cls.shape)
            b1, b2 = keystream(regs[on], count_of(FN[on]))
            ks[on] = b2 if uplink else b1
        return on, ks

    def bits(self, uplink, fn, F, bits, what=None, what_mask=0):
        """bits uint8 [A][8 F][148] -> the ciphered copy"""
        el = None if what is None else ((int(what_mask) >> np.minimum(what.astype(np.int64), 63)) & 1).astype(bool) & (what < 32)
        _, ks = self.slot_keystream(uplink, fn, F, el)
        out = np.array(bits, np.uint8)
        out[..., POS] ^= ks
        return out

    def soft(self, uplink, fn, row, valid, soft):
        """row int32 [T][A], valid uint8 [n_rows], soft float32 [n_rows][stride] -> the deciphered copy of soft"""
        T, A = row.shape
        on, ks = self.slot_keystream(uplink, fn, T // 8)
        out = np.array(soft, np.float32)
        for t in range(T):
            for a in range(A):
                r = int(row[t, a])
                if on[a, t] and 0 <= r < len(valid) and valid[r]:
                    p = POS[ks[a, t] != 0]
                    out[r, p] = np.float32(1.0) - out[r, p]
        return out
