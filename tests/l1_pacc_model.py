"""A literal model of packet access through L1 (include/trxsig_l1pacc.h) on the CPU -- TEST INFRASTRUCTURE ONLY.  The coder, the
Viterbi decoder, the parity and the UDP hop are the oracle's through tests/access_model.py; the detector and the demodulator
are the oracle's (oraclebind.Oracle.rach_batch); the CS-1 block of the timing-advance loop is tests/pdtch_model.py's.  What is
stated here: the frame rules, the block indexing, the table, the message, the reading of it and the TA formula in float32.

The frame rules (PTCCH/U on FN mod 416 = 12 + 26 n for TAI n; a PRACH block = four occasions) and the message's octets are
from memory of GSM 05.02 / 03.64 / 04.60, as the header says."""
import numpy as np

import access_model as am
import pdtch_model as pm

HYPERFRAME = 2715648
NONE, PTCCH, PRACH = 0, 1, 2
W_PACC = 9                                                  # TRXSIG_L1TX_PACC
STATE_BYTES = 144


def tai_of(fn):
    """The TAI whose PTCCH/U frame fn is, or -1."""
    return (fn % 416 - 12) // 26 if fn % 26 == 12 else -1


def block_of(fn):
    """(absolute block number within the hyperframe's count, entry 0..3) of a frame of a block B0..B11, or (-1, -1)."""
    b, t = pm.pdch_map(fn)
    return (12 * (fn // 52) + b, t) if b >= 0 else (-1, -1)


def blocks(fn, F):
    """(the first block with a frame in [fn, fn + F), how many have one): frames past the hyperframe count on, unwrapped."""
    seen = [block_of(u)[0] for u in range(fn, fn + F) if block_of(u)[0] >= 0]
    return (seen[0], seen[-1] - seen[0] + 1) if seen else (0, 0)


def pdchs(comb):
    """[(arfcn, tn)] in (ARFCN, TN) order"""
    return [(a, tn) for a in range(comb.shape[0]) for tn in range(8) if comb[a, tn] == 13]


def ta_of(toa, sps):
    t = np.float32(toa) / np.float32(sps)
    return 0 if t < 0 else min(63, int(np.float32(t + np.float32(0.5))))


def occasion(fn, F, k, g, prach):
    """What frame k of a call is for PDCH g: (kind, tai); prach [n, nb] or None."""
    u = fn + k
    if tai_of(u) >= 0:
        return PTCCH, tai_of(u)
    blk, _ = block_of(u)
    if blk >= 0 and prach is not None and prach[g, blk - blocks(fn, F)[0]]:
        return PRACH, -1
    return NONE, -1


def encode(o, comb, bsic, fn, F, ptcch_kind, ptcch_ra, prach_kind, prach_ra, fmt, onto=None):
    """-> bits [A, 8 F, 148], what [A, 8 F]; onto: (bits, what) to overlay."""
    A = comb.shape[0]
    bits, what = (np.zeros((A, 8 * F, 148), np.uint8), np.zeros((A, 8 * F), np.uint8)) if onto is None else (onto[0].copy(), onto[1].copy())
    blk0, _ = blocks(fn, F)
    for g, (a, tn) in enumerate(pdchs(comb)):
        for k in range(F):
            u = fn + k
            if tai_of(u) >= 0:
                kind, ra = ptcch_kind[g, tai_of(u)], ptcch_ra[g, tai_of(u)]
            else:
                blk, t = block_of(u)
                if blk < 0:
                    continue
                kind, ra = prach_kind[g, blk - blk0, t], prach_ra[g, blk - blk0, t]
            if kind == 1 and am.fits(int(ra), fmt, bsic):
                bits[a, 8 * k + tn] = am.encode(o, [int(ra)], [fmt], [bsic])[0]
                what[a, 8 * k + tn] = W_PACC
    return bits, what


class Table:
    """The PDCHs' records: ta, fn (int32 [n, 16]) and valid (uint8 [n, 16])."""

    def __init__(self, n):
        self.ta, self.fn, self.valid = np.zeros((n, 16), np.int32), np.zeros((n, 16), np.int32), np.zeros((n, 16), np.uint8)

    def same(self, s):
        return all(np.array_equal(getattr(self, k), s[k]) for k in ("ta", "fn", "valid"))

    def message(self, nb_pt):
        n = self.ta.shape[0]
        payload = np.full((n, nb_pt, 23), 0x2B, np.uint8)
        payload[:, :, :16] = np.where(self.valid != 0, self.ta & 0x7F, 0x7F).astype(np.uint8)[:, None, :]
        return np.ones((n, nb_pt), np.uint8), payload


def ta_read(ta, payload, ok):
    """ta [n, 16] <- octets 0..15 of the latest block with ok, per PDCH, where they hold a value; unchanged elsewhere."""
    ta = ta.copy()
    for g in range(ta.shape[0]):
        for b in range(ok.shape[1] - 1, -1, -1):
            if ok[g, b]:
                v = payload[g, b, :16]
                ta[g] = np.where(v <= 63, v, ta[g])
                break
    return ta


def cell_list(comb, fn, F, prach, sps, slot_stride, arfcn_stride):
    """The occasions in the library's order: (g, k, kind, offset, length) lists."""
    out = []
    for g, (a, tn) in enumerate(pdchs(comb)):
        for k in range(F):
            kind, _ = occasion(fn, F, k, g, prach)
            if kind:
                out.append((g, k, kind, (8 * k + tn) * slot_stride + a * arfcn_stride, (156 + (tn % 4 == 0)) * sps))
    return out


def fold(fo, table, comb, bsic, fn, F, prach, sps, occ, det, amp, toa, avgpwr, soft, fmt, wire):
    """The detector's results per occasion (det, amp, toa, avgpwr, soft [n_occ, 148]) -> the dense outputs; updates table."""
    n = len(pdchs(comb))
    r = dict(kind=np.zeros((n, F), np.uint8), tai=np.full((n, F), -1, np.int8), det=np.zeros((n, F), np.uint8),
             fmt=np.zeros((n, F), np.uint8), ok=np.zeros((n, F), np.uint8), ra=np.zeros((n, F), np.uint16),
             amp=np.zeros((n, F), np.complex64), toa=np.zeros((n, F), np.float32), avgpwr=np.zeros((n, F), np.float32),
             ta=np.zeros((n, F), np.uint8))
    if not occ:
        return r
    ra, f, tail, b = am.decode(fo, soft, None, len(occ), wire=wire, fmt=fmt, bsic=bsic)
    for i, (g, k, kind, _, _) in enumerate(occ):
        u = fn + k
        r["kind"][g, k], r["tai"][g, k] = kind, tai_of(u) if kind == PTCCH else -1
        r["amp"][g, k], r["toa"][g, k], r["avgpwr"][g, k] = amp[i], toa[i], avgpwr[i]
        if not det[i]:
            continue
        ok = bool(tail[i]) and b[i] == bsic
        r["det"][g, k], r["fmt"][g, k], r["ok"][g, k], r["ra"][g, k], r["ta"][g, k] = 1, f[i], ok, ra[i], ta_of(toa[i], sps)
        if ok and kind == PTCCH:
            t = tai_of(u)
            table.ta[g, t], table.fn[g, t], table.valid[g, t] = ta_of(toa[i], sps), u % HYPERFRAME, 1
    return r


def detect(fo, so, table, comb, bsic, cells, slot_stride, arfcn_stride, fn, F, prach, fmt, wire, thresh=5.0):
    """The base-station side on host cells (complex64, flat) through the oracle's detectRACHBurst and demodulateBurst.  avgpwr is
    not the oracle's to give here: the caller compares it elsewhere (zeros)."""
    occ = cell_list(comb, fn, F, prach, so.sps, slot_stride, arfcn_stride)
    if not occ:
        return fold(fo, table, comb, bsic, fn, F, prach, so.sps, occ, [], [], [], [], None, fmt, wire)
    off, length = [c[3] for c in occ], [c[4] for c in occ]
    ok, amp, toa, soft = so.rach_batch(cells, off, length, thresh=thresh, nthreads=4)
    return fold(fo, table, comb, bsic, fn, F, prach, so.sps, occ, ok, amp, toa, np.zeros(len(occ), np.float32), soft, fmt, wire)


# ---- the closed-loop inputs that tests/test_l1_pacc_model.py (CPU, the oracle's modulator) and tests/test_gpu_l1pacc.py (the
#      card's) share: the same plan, seeds, words, delays and level ----
COMB = np.array([[5, 13, 1, 13, 1, 1, 7, 1], [1, 1, 13, 1, 0, 1, 1, 1]], np.uint8)   # 2 ARFCNs, 3 PDCHs among circuit slots
BSIC, AMPLITUDE, CELL_SYMBOLS, MAX_DELAY = 0x2B, 1000.0, 160, 20


def delays(rng, shape):
    """Whole and fractional delays of 0..MAX_DELAY symbols, no fraction within 0.2 of a half (the TA rounds them)."""
    d = rng.integers(0, MAX_DELAY + 1, shape) + rng.choice(np.array([0.0, 0.0, 0.125, 0.25, 0.75, 0.875]), shape)
    return np.minimum(d, MAX_DELAY).astype(np.float32)


def scenario(seed, fn, F, fmt, p_ptcch=0.7, p_prach=0.5):
    """Random handset inputs for the three PDCHs: dict(ptcch_kind, ptcch_ra, ptcch_delay [n, 16]; prach_kind, prach_ra,
    prach_delay [n, nb, 4]; prach [n, nb]: the blocks the base station marks -- every block with a burst and some without)."""
    rng = np.random.default_rng(seed)
    n, nb = len(pdchs(COMB)), blocks(fn, F)[1]
    top = 2048 if fmt else 256
    marked = rng.random((n, nb)) < p_prach
    s = dict(ptcch_kind=(rng.random((n, 16)) < p_ptcch).astype(np.uint8), ptcch_ra=rng.integers(0, top, (n, 16)).astype(np.uint16),
             ptcch_delay=delays(rng, (n, 16)), prach_ra=rng.integers(0, top, (n, nb, 4)).astype(np.uint16),
             prach_delay=delays(rng, (n, nb, 4)))
    s["prach_kind"] = ((rng.random((n, nb, 4)) < 0.6) & marked[:, :, None]).astype(np.uint8)
    s["prach"] = (marked | (rng.random((n, nb)) < 0.15)).astype(np.uint8)
    return s


def sent_bursts(s, fn, F):
    """[(g, k, ra, delay)] of the bursts the scenario's handsets send in the call."""
    out = []
    blk0, _ = blocks(fn, F)
    for g in range(len(pdchs(COMB))):
        for k in range(F):
            u = fn + k
            if tai_of(u) >= 0:
                t = tai_of(u)
                if s["ptcch_kind"][g, t] == 1:
                    out.append((g, k, int(s["ptcch_ra"][g, t]), float(s["ptcch_delay"][g, t])))
            else:
                blk, t = block_of(u)
                if blk >= 0 and s["prach_kind"][g, blk - blk0, t] == 1:
                    out.append((g, k, int(s["prach_ra"][g, blk - blk0, t]), float(s["prach_delay"][g, blk - blk0, t])))
    return out


def cells_cpu(fo, so, s, fn, F, fmt):
    """The uplink slot cells through the oracle's modulator, delayVector and scaleVector: (cells, slot_stride, arfcn_stride)."""
    A, cell = COMB.shape[0], CELL_SYMBOLS * so.sps
    x = np.zeros(8 * F * A * cell, np.complex64)
    ch = pdchs(COMB)
    for g, k, ra, delay in sent_bursts(s, fn, F):
        a, tn = ch[g]
        bits = am.encode(fo, [ra], [fmt], [BSIC])[0]
        y = so.scale_vector(so.delay_vector(so.modulate(bits, 8 + (tn % 4 == 0)), np.float32(delay) * np.float32(so.sps)), AMPLITUDE)
        o = ((8 * k + tn) * A + a) * cell
        x[o:o + y.size] = y
    return x, A * cell, cell
