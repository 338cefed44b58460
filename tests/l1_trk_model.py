"""The literal model of the handset's tracking receiver (include/trxsig_l1trk.h): python integers for the anchor, the NCO and the
timing rule, the oracle's expjLookup and Complex<float> product for the cells, float64 for the FCCH sums C and E -- and the closed
loop both tests/test_l1_trk_model.py (this model with the reference's detectors) and tests/test_gpu_l1trk.py (the device) run:
one seeded cell, one phone with two columns whose two clocks drift.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import air_model as am
import l1_msrx_model as lrm
import l1_mux_model as lmm

HYPER = am.HYPER
M32 = 0xffffffff
F32 = np.float32
K_TURN = 4294967296.0 / 6.283185307179586
CLIPPED, UNLOCKED = 1, 2
FCCH_T3, SCH_T3 = (0, 10, 20, 30, 40), (1, 11, 21, 31, 41)


def cell_start(t, sps):
    """s_t: the stream offset of cell t, the sum of the lengths of the cells before it (157 / 156 / 156 / 156)"""
    return (t // 4) * 625 * sps + ((157 + 156 * (t % 4 - 1)) * sps if t % 4 else 0)


def distance(fn_from, fn_to):
    """the signed shortest distance modulo the hyperframe"""
    d = (fn_to - fn_from) % HYPER
    return d - HYPER if d >= HYPER // 2 else d


def timing_adj(S, N, sps):
    """floor((2 S sps + 256 N) / (512 N)): S sps / (256 N) samples, rounded half up"""
    return (2 * S * sps + 256 * N) // (512 * N)


def quantise_toa(toa, sps):
    """q = llrint((double) toa * (256 / sps)): round half to even, as the default rounding mode does"""
    return int(np.rint(np.float64(F32(toa)) * (256 // sps)))


def timing_excluded(fn, t, is_c0):
    """the C0 column's TN 0 in an FCCH or SCH frame"""
    return is_c0 and t % 8 == 0 and ((fn + t // 8) % HYPER) % 51 in FCCH_T3 + SCH_T3


def expj_many(o, top):
    """expjLookup((float) top * 2^-24f * (float)(2 pi)) for an array of 24-bit phases: sigProcLib.cpp:192-204 in float32 numpy on
    the oracle's own tables (tests/test_l1_trk_model.py holds it to the oracle's scalar function word for word)"""
    x = (np.asarray(top).astype(F32) * F32(2.0 ** -24)) * am.TWO_PI_F
    arg = x * (F32(1) / am.TWO_PI_F)
    arg = np.where(arg > F32(1), arg - (np.ceil(arg) - F32(1)), arg).astype(F32)
    argT = arg * F32(1024)
    argI = argT.astype(np.int32)
    delta = argT - argI.astype(F32)
    iD = F32(1) - delta
    out = np.empty(len(x), np.complex64)
    out.real = iD * o.cosT[argI] + delta * o.cosT[argI + 1]
    out.imag = iD * o.sinT[argI] + delta * o.sinT[argI + 1]
    return out


class TrkModel:
    def __init__(self, o, phone, c0, afc_shift=1, toa_gate=512, fcch_thresh=0.5):
        self.o, self.sps = o, o.sps
        self.phone, self.c0 = [int(p) for p in phone], [int(c) for c in c0]
        self.P, self.C = len(self.c0), len(self.phone)
        self.afc_shift, self.toa_gate, self.fcch_thresh = afc_shift, toa_gate, float(F32(fcch_thresh))
        self.fn, self.pos, self.phase, self.step = [0] * self.P, [0] * self.P, [0] * self.P, [0] * self.P
        self.locked, self.quiet = [0] * self.P, [0] * self.P
        self.last = None                                         # (fn, n_frames, records) of the last slice
        self.did = None                                          # what the last update did

    def set(self, p, locked, fn, pos, step, phase):
        self.locked[p], self.fn[p], self.pos[p], self.step[p], self.phase[p], self.quiet[p] = int(bool(locked)), fn, pos, step & M32, phase & M32, 0

    def seed(self, acq, src):
        """acq: dict(state, sch_w0, sch_toa, omega, rfn) of arrays, one entry per stream; src[p]: the phone's stream, -1: leave"""
        for p, s in enumerate(src):
            if s < 0 or s >= len(acq["state"]):
                continue
            if int(acq["state"][s]) != 15:
                self.locked[p] = 0
                continue
            pos0 = int(np.floor(float(acq["sch_w0"][s]) + float(F32(acq["sch_toa"][s])) + 0.5))
            self.set(p, 1, (int(acq["rfn"][s]) + 1) % HYPER, pos0 + 1250 * self.sps,
                     int(np.rint(float(F32(acq["omega"][s])) * K_TURN)) & M32, 0)

    def moved(self, p, fn):
        """(P, PH): the anchor moved to frame fn"""
        shift = distance(self.fn[p], fn) * 1250 * self.sps
        return self.pos[p] + shift, (self.phase[p] + (shift & M32) * self.step[p]) & M32

    def slice(self, streams, n0, fn, n_frames):
        """streams: [n_cols][n_samples] complex64 holding the absolute samples [n0, n0 + n_samples).  Returns (cells [c][t],
        status [n_cols], records [p] -> list of dict(fn, C, E, ok)) and advances the anchors."""
        sps, T = self.sps, 8 * n_frames
        streams = np.asarray(streams, np.complex64)
        n_samples = streams.shape[1]
        cells, status = [], []
        rec = [[] for _ in range(self.P)]
        for c in range(self.C):
            p = self.phone[c]
            row = []
            if not self.locked[p]:
                status.append(UNLOCKED)
                cells.append([np.zeros(am.cell_len(t, sps), np.complex64) for t in range(T)])
                if self.c0[p] == c:
                    rec[p] = [dict(fn=(fn + f) % HYPER, C=0j, E=0.0, ok=False) for f in range(n_frames) if ((fn + f) % HYPER) % 51 in FCCH_T3]
                continue
            Pp, PH = self.moved(p, fn)
            span = n_frames * 1250 * sps
            q = Pp - n0 + np.arange(span, dtype=np.int64)
            ok = (q >= 0) & (q < n_samples)
            x = np.zeros(span, np.complex64)
            x[ok] = streams[c][q[ok]]
            ph = (PH + np.arange(span, dtype=np.uint64) * np.uint64(self.step[p])) & np.uint64(M32)
            y = am.cmul32(x, expj_many(self.o, (ph >> np.uint64(8)).astype(np.int64)))
            y[~ok] = 0                                           # (+0, +0) where nothing was read
            status.append(CLIPPED if not ok.all() else 0)
            for t in range(T):
                row.append(y[cell_start(t, sps):cell_start(t, sps) + am.cell_len(t, sps)].copy())
            cells.append(row)
            if self.c0[p] == c:
                for f in range(n_frames):
                    if ((fn + f) % HYPER) % 51 in FCCH_T3:
                        rec[p].append(dict(fn=(fn + f) % HYPER, **self.fcch(row[8 * f])))
        for p in range(self.P):
            if self.locked[p]:
                Pp, PH = self.moved(p, fn)
                span = n_frames * 1250 * sps
                self.fn[p], self.pos[p], self.phase[p] = (fn + n_frames) % HYPER, Pp + span, (PH + (span & M32) * self.step[p]) & M32
        self.last = (fn, n_frames, rec)
        return cells, status, rec

    def fcch(self, y):
        """C, E over n = 3 sps .. 3 sps + 142 sps - 1 of a derotated TN 0 cell, in float64, and the acceptance rule"""
        sps = self.sps
        y = np.asarray(y, np.complex64).astype(np.complex128)
        n = 3 * sps + np.arange(142 * sps)
        with np.errstate(all="ignore"):
            C = complex(np.sum(y[n + sps] * np.conj(y[n]) * (-1j)))
            E = float(np.sum(0.5 * (np.abs(y[n]) ** 2 + np.abs(y[n + sps]) ** 2)))
            ok = bool(C.real > 0 and E > 0 and np.isfinite([C.real, C.imag, E]).all() and abs(C) ** 2 / E ** 2 > self.fcch_thresh)
        return dict(C=C, E=E, ok=ok, bound_c=float(4 * 2.0 ** -24 * np.sum(np.abs(y[n + sps]) * np.abs(y[n]))),
                    bound_e=float(4 * 2.0 ** -24 * E))

    def update(self, row, valid, toa, fn, use=None):
        """row [n_slots][n_cols] (-1: none), valid / toa [n_rows]: a pull's result; fn: the last slice's"""
        lfn, n_frames, rec = self.last
        assert fn == lfn and np.shape(row) == (8 * n_frames, self.C)
        sps = self.sps
        self.did = []
        for p in range(self.P):
            if not self.locked[p]:
                self.did.append(dict(S=0, N=0, adj=0, K=0, delta=0))
                continue
            S = N = 0
            for t in range(8 * n_frames):
                for c in range(self.C):
                    if self.phone[c] != p:
                        continue
                    r = int(row[t][c])
                    if r < 0 or not valid[r] or (use is not None and not use[t][c]) or timing_excluded(fn, t, self.c0[p] == c):
                        continue
                    if not np.isfinite(toa[r]):
                        continue
                    q = quantise_toa(toa[r], sps)
                    if abs(q) > self.toa_gate:
                        continue
                    S, N = S + q, N + 1
            adj = 0
            if N >= 1:
                adj = timing_adj(S, N, sps)
                self.pos[p] += adj
                self.phase[p] = (self.phase[p] + (adj & M32) * self.step[p]) & M32
            good = [r["C"] for r in rec[p] if r["ok"]]
            K, delta = len(good), 0
            if K >= 1:
                sc = sum(good)
                a = float(F32(np.arctan2(F32(sc.imag), F32(sc.real))))
                delta = int(np.rint(-a / sps * K_TURN))
                self.step[p] = (self.step[p] + (delta >> self.afc_shift)) & M32
            self.quiet[p] = 0 if N + K > 0 else self.quiet[p] + 1
            self.did.append(dict(S=S, N=N, adj=adj, K=K, delta=delta))
        self.last = None
        return self.did


# ---- the closed loop ----------------------------------------------------------------------------------------------------------
LOOP_SPS, LOOP_FRAMES, LOOP_ROUNDS, LOOP_ROUND_FRAMES = 4, 120, 6, 17
LOOP_SNR_DB = 30.0                                           # tests/air_loops.py's level where every unprotected bit comes back
LOOP_MARGIN = 64                                             # samples of stream either side of a round's nominal span
MAX_SEED, MAX_GRID = 0.75, 1.0                               # samples: 0.5 rounding + 0.25 acquisition; 0.5 + 0.2 drift + 0.3 TOA
SCH_LEAD = 4                                                 # symbols of zeros in front of an SCH cell's detector window


def loop_case(tx):
    """tm.PLAN over 120 frames through l1tx's model, one phone that hears both carriers (column c = ARFCN c, C0 = column 0): a
    cut inside the first ten frames (drawn again by tests/air_loops.py's orphan rule), a delay in [0, 1) sample that grows by
    0.2 sample per round, an offset within +-0.02 cycle / symbol that moves by 1e-3 over the six rounds, a gain of 1000 (the
    group's energy gate starts at 250), 30 dB."""
    import test_l1_msrx_model as tm
    sps = LOOP_SPS
    rng = np.random.default_rng(7300)
    bsic, band, fn0, F = 45, 900, 51 * 26 * 23, LOOP_FRAMES
    mux, enc, grids = tm.encode_cell(rng, tx, fn0, F, bsic, band)
    T = 8 * F
    starts = np.concatenate([[0], np.cumsum([am.cell_len(t, sps) for t in range(T)])])
    fcch = [int(starts[t]) for t in range(T) if enc["what"][0, t] == lmm.W_FCCH]
    n = 12 * 1250 * sps + 313 * sps

    def orphan(c):
        return any(c - 48 * sps <= p and p + 100 * sps <= c + n < p + (1250 + 172) * sps for p in fcch)
    while True:
        cut = int(rng.integers(0, 10 * 1250 * sps))
        if not orphan(cut):
            break
    f0 = float(rng.uniform(-0.02, 0.02))
    f = [f0 + 1e-3 * r / LOOP_ROUNDS for r in range(LOOP_ROUNDS + 1)]           # entry 0: the search; entry r: round r (1-based)
    step = [int(round(v / sps * 2.0 ** 32)) & M32 for v in f]
    d0 = float(rng.uniform(0, 1))
    delay = [F32(d0 + 0.2 * r) for r in range(LOOP_ROUNDS + 1)]
    gain = np.complex64(1000.0 * np.exp(2j * np.pi * rng.uniform()))
    sigma = F32(abs(gain) * 10.0 ** (-LOOP_SNR_DB / 20.0) / np.sqrt(2.0))
    return dict(sps=sps, bsic=bsic, band=band, fn0=fn0, F=F, mux=mux, enc=enc, grids=grids, starts=starts, n=n, cut=cut, f=f, step=step,
                delay=delay, gain=gain, sigma=sigma, phase0=int(rng.integers(0, 1 << 32)), noise0=int(rng.integers(0, 1 << 32)),
                seed=0x7a11c0de)


def true_start(case, fn, r):
    """where TN 0 of frame fn truly starts in absolute stream samples, under round r's delay"""
    k = fn - case["fn0"]
    return float(case["starts"][8 * k]) - case["cut"] + float(case["delay"][r])


def true_step(case, r):
    """the step that undoes round r's offset exactly"""
    return (-case["step"][r]) & M32


def step_error(case, r, step):
    """|residual offset| in cycles / symbol of an NCO step against round r's oscillator"""
    e = (step + case["step"][r]) & M32
    e = e - (1 << 32) if e >= 1 << 31 else e
    return abs(e) / 2.0 ** 32 * case["sps"]


def round_plan(case, pos, r):
    """the buffer of round r (1-based) given the tracker's anchor position before it: (n0, n_samples)"""
    return pos - LOOP_MARGIN, LOOP_ROUND_FRAMES * 1250 * case["sps"] + 2 * LOOP_MARGIN


class LoopAir:
    """the oscillator and the noise counter of the one continuous signal: phase and n0 are carried from buffer to buffer"""

    def __init__(self, case):
        self.case, self.at, self.phase = case, 0, case["phase0"]

    def params(self, r, n0):
        """stream-form parameters of a buffer that starts at absolute sample n0 >= the previous buffer's start, round r's step"""
        case = self.case
        prev = case["step"][max(r - 1, 0)]
        self.phase = (self.phase + ((n0 - self.at) & M32) * prev) & M32
        self.at = n0
        return dict(cut=case["cut"] + n0, delay=case["delay"][r], step=case["step"][r], phase=self.phase, n0=(case["noise0"] + n0) & M32)


def merge_outputs(outs):
    """the decoder's outputs of consecutive calls as one: the block arrays side by side, a row's decoded blocks first (a call
    also lists closing frames beyond its span, with status 0)"""
    out = {}
    for key in ("tch", "xcch", "ccch", "bcch"):
        cat = {k: np.concatenate([o[key][k] for o in outs], axis=1) for k in ("status", "frames", "facch", "fn", "tc") if k in outs[0][key]}
        for i in range(cat["status"].shape[0]):
            order = np.argsort(cat["status"][i] == 0, kind="stable")
            for k in cat:
                cat[k][i] = cat[k][i][order]
        out[key] = cat
    return out


def check_span(model, out, mux, grids, case, lo, hi):
    """test_l1_msrx_model.check_payloads for the blocks that lie wholly inside the tracked frames [lo, hi) of an encode that
    began at case["fn0"]: the same assertions, the block index counted from the encode's first frame"""
    import fec_stream_model as fsm
    import test_l1_msrx_model as tm
    n = dict(tch=0, xcch=0, ccch=0, bcch=0)
    cls_of = {lmm.TCH: lrm.TCH, lmm.XCCH: lrm.XCCH, lmm.CCCH: lrm.CCCH, lmm.BCCH: lrm.BCCH}
    for (cls, i, b), first in tm.sent_blocks(mux, case["fn0"], case["F"]).items():
        key = lrm.KEYS[cls_of[cls]]
        c = model.ch[cls_of[cls]][i]
        o = out[key]
        closing = model.next_closing(c, model.next_closing(c, first) + 1) if cls == lmm.TCH else model.next_closing(c, first)
        if first < lo or closing >= hi:
            continue
        col = list(o["fn"][i]).index(closing % HYPER)
        st = int(o["status"][i, col])
        if cls == lmm.TCH:
            if grids["tch_kind"][i, b] == 1:
                assert st == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(o["frames"][i, col], grids["tch_payload"][i, b]), (i, b)
            else:
                assert st & fsm.FACCH_OK and np.array_equal(o["facch"][i, col], grids["tch_payload"][i, b, :23]), (i, b)
        else:
            assert st == fsm.DECODED | fsm.TCH_GOOD, (key, i, b, st)
            fr = o["frames"][i, col]
            if cls == lmm.BCCH:
                tc = ((first % HYPER) // 51) % 8
                assert o["tc"][i, col] == tc and np.array_equal(fr, mux.si[lmm.SI_OF_TC[tc]]), (i, b)
            else:
                want = grids["xcch_payload" if cls == lmm.XCCH else "ccch_payload"][i, b]
                assert np.array_equal(fr[2:], want[2:]), (key, i, b)
                if not c.sacch:
                    assert np.array_equal(fr[:2], want[:2])
        n[key] += 1
    return n
