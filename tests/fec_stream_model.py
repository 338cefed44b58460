"""A literal restatement of the uplink stream decoders (trxsig_fec_tch_decode_stream / trxsig_fec_xcch_decode_stream) on the
CPU -- TEST INFRASTRUCTURE ONLY.  Each channel is the reference's decoder object, driven one burst at a time:

  TCHFACCHL1Decoder::processBurst / deinterleave / decodeTCH (GSM/GSML1FEC.cpp:1030-1163)
  XCCHL1Decoder::writeLowSide / processBurst / deinterleave / decode (:556-653)
  L1Decoder::countGoodFrame / countBadFrame (:390-405)

with mI[][] as float32 rows (a fresh decoder: all 0.0), 0.5F marking every position a deinterleave consumes, a block decoded
only when its closing burst (B % 4 == 3) arrives, and the FER recurrence in float32.  The decode primitives are the existing
oracle's (oracle/fecbind.py: viterbi_decode, syndrome, lsb8msb, wire, tch_decode); where the real reference's coder has been
built (oracle/_ref/libref_fec.so) its own tch_decode / xcch_decode run instead.  No closed form here: the device's is checked
against this."""
import numpy as np

import fecbind
import reffec

TCH_STATE_BYTES, XCCH_STATE_BYTES = 3664, 1840
DECODED, STOLEN, FACCH_OK, TCH_GOOD = 1, 2, 4, 8
HDR = 16
XCCH_POLY = 0x10004820009

_K = np.arange(456)
_J = 2 * ((49 * _K) % 57) + ((_K % 8) // 4)                 # GSM 05.03 3.1.3 / 4.1.4 (fec:622-625, 1111)
_E = np.r_[3:60, 88:145]                                     # data1 / data2: the burst's e-bits (fec:607-608)
_FA = np.float32(1.0) / np.float32(20.0)                     # mFERMemory = 20
_FB = np.float32(1.0) - _FA


class Prims:
    """The decode primitives: the CPU oracle's, or the reference's own coder where it has been built."""

    def __init__(self, use_ref=None):
        self.fo = fecbind.FecOracle()
        self.ref = reffec.RefFec() if (reffec.available() if use_ref is None else use_ref) else None

    def wire(self, v):
        return self.fo.wire(v)

    def xcch(self, c456):
        """XCCHL1Decoder::decode on c[] + mD.LSB8MSB(): (ok, the 23-octet L2 frame)."""
        c = np.asarray(c456, np.float32)
        if self.ref is not None:
            i4 = np.zeros((4, 114), np.float32)              # the XCCH deinterleaver's inverse: its c[] is this c[]
            i4[_K % 4, _J] = c
            r = self.ref.xcch_decode(i4)
            return r["ok"], pack(r["d"], 23)
        u = self.fo.viterbi_decode(c, 228)
        dp = u[:224].copy()
        dp[184:] ^= 1                                        # mP.invert() (fec:644)
        ok = self.fo.syndrome(XCCH_POLY, 40, dp) == 0
        return ok, pack(self.fo.lsb8msb(u[:184]), 23)

    def tch(self, c456):
        """decodeTCH(false) up to `good`: (good, d[260] packed MSB first in 33 octets)."""
        r = (self.ref or self.fo).tch_decode(np.asarray(c456, np.float32))
        return r["good"], pack(r["d"], 33)


def pack(bits, n_octets):
    b = np.zeros(8 * n_octets, np.uint8)
    b[:len(bits)] = np.asarray(bits, np.uint8) & 1
    return np.packbits(b)


class Decoder:
    """One channel's decoder.  tch: TCHFACCHL1Decoder (8 rows), else XCCHL1Decoder (4 rows)."""

    def __init__(self, prims, tch, state=None):
        self.p, self.tch = prims, tch
        self.rows = 8 if tch else 4
        self.mI = np.zeros((self.rows, 114), np.float32)     # fill(0.0)
        self.fer = np.float32(0.0)
        if state is not None:
            st = np.asarray(state, np.uint8)
            self.fer = st[:4].view(np.float32)[0]
            self.mI = st[HDR:].view(np.float32).reshape(self.rows, 114).copy()

    def state(self):
        out = np.zeros(HDR + self.rows * 114 * 4, np.uint8)
        out[:4] = np.array([self.fer], np.float32).view(np.uint8)
        out[HDR:] = self.mI.astype(np.float32).view(np.uint8).ravel()
        return out

    def count(self, good):
        if good:
            self.fer = np.float32(self.fer * _FB)
        else:
            self.fer = np.float32(np.float32(_FB * self.fer) + _FA)

    def deinterleave(self, offset):
        B = (_K + offset) % 8 if self.tch else _K % 4
        c = self.mI[B, _J].copy()
        self.mI[B, _J] = np.float32(0.5)
        return c

    def burst(self, B, v):
        """processBurst for a burst at index B with soft values v[148] (already through the wire hop).  Returns None (no block
        closes) or (status, tch33, l2_23)."""
        self.mI[B, :] = v[_E]
        if B % 4 != 3:
            return None
        tch33, l2 = np.zeros(33, np.uint8), np.zeros(23, np.uint8)
        if not self.tch:
            c = self.deinterleave(0)
            ok, l2 = self.p.xcch(c)
            self.count(ok)
            return DECODED | (TCH_GOOD if ok else 0), tch33, l2
        c = self.deinterleave(4 if B == 3 else 0)
        stolen = v[60] > np.float32(0.5)                     # Hl (fec:1077)
        st = DECODED
        if stolen:
            ok, l2 = self.p.xcch(c)
            self.count(ok)
            st |= STOLEN | (FACCH_OK if ok else 0)
            self.count(False)                                # decodeTCH(true) returns false
        else:
            good, tch33 = self.p.tch(c)
            self.count(good)
            st |= TCH_GOOD if good else 0
        return st, tch33, l2


def run(prims, tch, soft, index, state, b0=None, wire=True):
    """The stream decoder on the host: soft[n_rows, >= 148] float32, index[S, T] (T % 4 == 0), state[S, bytes] uint8, b0[S]
    (TCH).  Returns dict(status[S, T/4], tch[S, T/4, 33] (TCH), l2[S, T/4, 23], fer[S, T/4], state[S, bytes])."""
    soft = np.asarray(soft, np.float32)
    index = np.asarray(index, np.int64)
    S, T = index.shape
    nb = T // 4
    out = dict(status=np.zeros((S, nb), np.uint8), tch=np.zeros((S, nb, 33), np.uint8), l2=np.zeros((S, nb, 23), np.uint8),
               fer=np.zeros((S, nb), np.float32), state=np.zeros((S, TCH_STATE_BYTES if tch else XCCH_STATE_BYTES), np.uint8))
    wired = {}
    for s in range(S):
        d = Decoder(prims, tch, state[s])
        bs = 0 if (b0 is None or not tch) else int(b0[s])
        chan_ok = not tch or bs in (0, 4)
        for t in range(T):
            i = int(index[s, t])
            if chan_ok and 0 <= i < soft.shape[0]:
                if i not in wired:
                    wired[i] = prims.wire(soft[i, :148]) if wire else soft[i, :148].copy()
                r = d.burst((bs + t) % 8 if tch else t % 4, wired[i])
                if r is not None:
                    out["status"][s, t // 4], out["tch"][s, t // 4], out["l2"][s, t // 4] = r
            if t % 4 == 3:
                out["fer"][s, t // 4] = d.fer
        out["state"][s] = d.state()
    return out


# ---- stream generators shared by the CPU and GPU tests ----
def soft_from_bits(rng, bits, noise=0.25):
    """Soft values for hard bits: 0.1 / 0.9 plus uniform noise, clipped to [0, 1], float32."""
    v = np.where(np.asarray(bits) != 0, 0.9, 0.1) + rng.uniform(-noise, noise, np.shape(bits))
    return np.clip(v, 0.0, 1.0).astype(np.float32)


def tch_bursts(rng, tx, S, n, p_facch=0.25, noise=0.25, p_junk=0.0):
    """S channels x n blocks of speech / FACCH through the literal TCH encoder (oracle/fectxbind.py): the soft bursts
    [S, 4n, 148] (a fraction p_junk of them replaced by uniform noise), the kinds [S, n] and the payloads [S, n, 33]."""
    kind = np.where(rng.random((S, n)) < p_facch, 2, 1).astype(np.uint8)
    pl = rng.integers(0, 256, (S, n, 33)).astype(np.uint8)
    pl[:, :, 32] &= 0xF0
    bits, _ = tx.tch_encode_stream(kind, pl, np.full(S, 3, np.uint8), np.zeros(456, np.uint8))
    soft = soft_from_bits(rng, bits.reshape(S, 4 * n, 148), noise)
    junk = rng.random((S, 4 * n)) < p_junk
    soft[junk] = rng.random((int(junk.sum()), 148)).astype(np.float32)
    return soft, kind, pl


def xcch_bursts(rng, fo, S, n, noise=0.25):
    """S channels x n XCCH blocks of random L2 frames: the soft bursts [S, 4n, 148] and the frames [S, n, 23]."""
    fr = rng.integers(0, 256, (S, n, 23)).astype(np.uint8)
    tsc = np.zeros(26, np.uint8)
    bits = np.stack([np.concatenate([fo.xcch_encode(fr[s, m], tsc) for m in range(n)]) for s in range(S)])
    return soft_from_bits(rng, bits, noise), fr
