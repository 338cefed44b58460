"""A model of mobile-side acquisition (include/trxsig_l1acq.h) on the CPU -- TEST INFRASTRUCTURE ONLY.

  stage 1   the FCCH metric in float64, exactly as the header states it (THIS PROJECT'S OWN arithmetic: the reference, a base
            station, never looks for a frequency burst).  The library's float32 segment scans are graded against it within
            8 (L + 8) 2^-24.
  stage 2   the SCH detector and demodulator as a composition of the oracle's primitives (oraclebind.Oracle.modulate /
            scale_vector / correlate / peak_detect / frequency_shift / demodulate) and the valley rule of analyzeTrafficBurst
            restated in float32 scalars: the library must equal it bit for bit.
  decode    tests/l1_msrx_model.py's sch_decode.

and the stream builder the CPU and GPU tests share: frames of eight slots modulated with guard 8 + (TN % 4 == 0) and
concatenated, TN 0 carrying FCCH on the frames with FN % 51 in {0, 10, 20, 30, 40} and SCH on the frames after them, the other
slots random, dummy and alternating-bit bursts; then a cut-in point, a fractional delay, a rotation, a complex gain and noise."""
import numpy as np

import l1_msrx_model as lrm
from fectxbind import XTS_BITS
from l1_mux_model import DUMMY

HYPER = lrm.HYPERFRAME
FCCH_T3 = (0, 10, 20, 30, 40)
SCH_T3 = (1, 11, 21, 31, 41)
F32 = np.float32


def fcch_len(sps):
    return 142 * sps


def fcch_tol(sps):
    """the bound on |m - m64|: each float32 sum of at most L terms errs by at most L 2^-24 of E; m <= 1 picks up four such
    terms; the factor 2 covers forming d, e and the quotient"""
    return 8.0 * (fcch_len(sps) + 8) * 2.0 ** -24


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------
def _window_sums(v, L):
    """sum(v[k : k + L]) for every k in float64 WITHOUT A SUBTRACTION: per-segment inclusive suffix and prefix scans, a window is
    one suffix plus one prefix (the header's scheme).  A differenced running sum is not good enough for a reference even in
    float64: beside slots 90 dB up it errs by 1.9e-4 (sps 1) and 4.3e-4 (sps 4) on the metric of a quiet frequency burst --
    beyond fcch_tol -- where direct window sums and these scans agree to 1e-13."""
    n = len(v)
    nseg = (n + L - 1) // L + 1
    pad = np.zeros(nseg * L, v.dtype); pad[:n] = v
    seg = pad.reshape(nseg, L)
    pre = np.cumsum(seg, axis=1)
    suf = np.cumsum(seg[:, ::-1], axis=1)[:, ::-1]
    k = np.arange(n - L + 1)
    j, r = k // L, k % L
    return suf[j, r] + np.where(r > 0, pre[j + 1, np.maximum(r - 1, 0)], 0)


def fcch_metric64(x, sps):
    """(C[k], E[k], m[k]) for k in [0, N - sps - L], float64; empty where the stream has no window"""
    x = np.asarray(x).astype(np.complex128)
    L, N = fcch_len(sps), len(x)
    if N - sps < L:
        z = np.zeros(0)
        return z.astype(np.complex128), z, z
    with np.errstate(all="ignore"):
        d = x[sps:] * np.conj(x[:-sps]) * (-1j)
        e = 0.5 * (np.abs(x[:-sps]) ** 2 + np.abs(x[sps:]) ** 2)
        bad = ~(np.isfinite(d.real) & np.isfinite(d.imag) & np.isfinite(e))
        C, E = _window_sums(np.where(bad, 0, d), L), _window_sums(np.where(bad, 0, e), L)
        nb = np.concatenate([[0], np.cumsum(bad)])
        nbad = nb[L:] - nb[:-L]
        m = np.where((C.real > 0) & (E > 0) & (nbad == 0), np.abs(C) ** 2 / np.where(E > 0, E, 1) ** 2, 0.0)
    return C, E, m


def fcch_search64(x, sps, thresh=0.5):
    """the stream's answer: dict(k, m, C, E, arg, omega, found); k = -1 where there is no window"""
    C, E, m = fcch_metric64(x, sps)
    if len(m) == 0:
        return dict(k=-1, m=0.0, C=0j, E=0.0, arg=0.0, omega=0.0, found=False)
    k = int(np.argmax(m))                                     # the first of the largest
    arg = float(np.arctan2(C[k].imag, C[k].real))
    return dict(k=k, m=float(m[k]), C=C[k], E=float(E[k]), arg=arg, omega=-arg / sps, found=bool(m[k] > thresh))


def sch_window(k, sps):
    """(w0, n) of the SCH window behind an FCCH window that starts at k"""
    return k - 3 * sps + 1250 * sps - 12 * sps, 172 * sps


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------
def _norm2(z):
    return F32(z.imag) * F32(z.imag) + F32(z.real) * F32(z.real)        # Complex.h:119


def _cdiv(x, a):
    """Complex<float>::operator/ : x * a.inv() (Complex.h:85, 154-160)"""
    n = _norm2(a)
    ir, ii = F32(a.real) / n, -F32(a.imag) / n
    xr, xi = F32(x.real), F32(x.imag)
    return np.complex64(complex(xr * ir - xi * ii, xr * ii + xi * ir))


class SchDetector:
    def __init__(self, o):
        """o: oraclebind.Oracle(sps)"""
        self.o, self.sps = o, o.sps
        seq = o.modulate(XTS_BITS, 0)                          # modulateBurst(XTS, gsmPulse, 0, sps)
        self.seq = o.scale_vector(seq, -1 + 0j)                # the sequence starts at bit 42: j^42 = -1
        self.gain, self.toa, _ = o.peak_detect(o.correlate(self.seq, self.seq))
        self.fo = None

    def detect(self, x, omega, thresh=8.0):
        """one window -> dict(flags, amp, toa, ptm, soft[148]); flags 2 = detected, 128 = not processed"""
        o, sps = self.o, self.sps
        x = np.asarray(x, np.complex64)
        n = len(x)
        out = dict(flags=0, amp=np.complex64(0), toa=F32(0), ptm=F32(0), soft=np.zeros(148, F32))
        if n <= 0 or n > 256 * sps:
            out["flags"] = 128
            return out
        y = x if omega is None else o.frequency_shift(x, F32(omega), 0.0)[0]
        c = o.correlate(y, self.seq)
        peak, toa, _ = o.peak_detect(c)
        toa = F32(toa)
        bogus = not (toa >= 0 and toa <= F32(n))               # sigProcLib.cpp:964
        ptm, amp = F32(0), np.complex64(0)
        if not bogus:
            p = int(np.rint(toa))
            valley, num = F32(0), 0
            for i in range(2 * sps, 5 * sps + 1):              # :971-980, this order
                if p - i >= 0:
                    valley = valley + _norm2(c[p - i]); num += 1
                if p + i < n:
                    valley = valley + _norm2(c[p + i]); num += 1
            if num < 2:
                bogus = True
            else:
                rms = F32(np.float64(np.sqrt(F32(valley / F32(num)))) + 0.00001)     # :989
                ptm = F32(np.sqrt(_norm2(peak)) / rms)
                amp = _cdiv(peak, self.gain)
        toa_b = F32(F32(toa - self.toa) - F32(42 * sps))
        out.update(amp=amp, toa=toa_b, ptm=ptm)
        if not bogus and ptm > F32(thresh):
            fl0 = np.floor(toa_b)
            if fl0 >= 0 and int(fl0) + 148 * sps <= n:
                i0 = int(fl0)
                nd = min(156 * sps, ((n - i0) // sps) * sps)
                out["flags"] = 2
                out["soft"] = o.demodulate(y[i0:i0 + nd], amp, F32(toa_b - F32(fl0)))[:148].astype(F32)
        return out


def search_model(det, fo, x, fcch_thresh=0.5, sch_thresh=8.0, k=None, omega=None):
    """One stream through both stages.  k / omega given: stage 2 on the window and with the shift the library reported (the
    float64 stage 1 still fills the fcch entry)."""
    sps = det.sps
    f = fcch_search64(x, sps, fcch_thresh)
    if k is None:
        kk, om, found = f["k"], F32(f["omega"]), f["found"]
    else:
        kk, om = int(k), F32(omega)
        found = kk >= 0 and bool(fcch_metric64(x, sps)[2][kk] > fcch_thresh)
    r = dict(fcch=f, state=0, w0=0, sch=None, ok=False, bsic=0, rfn=0)
    if kk < 0 or not found:
        return r
    r["state"] = 1
    w0, n = sch_window(kk, sps)
    r["w0"] = w0
    if w0 < 0 or w0 + n > len(x):
        return r
    r["state"] |= 2
    s = det.detect(x[w0:w0 + n], om, sch_thresh)
    r["sch"] = s
    if s["flags"] & 2:
        r["state"] |= 4
    r["ok"], r["bsic"], r["rfn"] = lrm.sch_decode(fo, s["soft"])
    if r["ok"] and r["state"] & 4:
        r["state"] |= 8
    return r


def fcch_metric32_segments(x, sps, running=False):
    """m[k] by a float32 emulation: the header's scheme (per-segment inclusive prefix and suffix scans, a window = one suffix
    plus one prefix), or, running=True, one running prefix sum that is differenced -- the scheme the header rules out."""
    x = np.asarray(x, np.complex64)
    L, nd = fcch_len(sps), len(x) - sps
    a, b = x[sps:], x[:-sps]
    dr = (a.imag * b.real - a.real * b.imag).astype(F32)
    di = (-(a.real * b.real + a.imag * b.imag)).astype(F32)
    e = (F32(0.5) * ((b.real * b.real + b.imag * b.imag) + (a.real * a.real + a.imag * a.imag))).astype(F32)
    K = nd - L + 1
    out = []
    for v in (dr, di, e):
        if running:
            cs = np.concatenate([[F32(0)], np.cumsum(v, dtype=F32)])
            out.append((cs[L:] - cs[:-L]).astype(F32))
            continue
        nseg = (nd + L - 1) // L + 1
        pad = np.zeros(nseg * L, F32); pad[:nd] = v
        seg = pad.reshape(nseg, L)
        pre = np.cumsum(seg, axis=1, dtype=F32)
        suf = np.cumsum(seg[:, ::-1], axis=1, dtype=F32)[:, ::-1]
        k = np.arange(K)
        j, r = k // L, k % L
        w = suf[j, r] + np.where(r > 0, pre[j + 1, np.maximum(r - 1, 0)], F32(0))
        out.append(w.astype(F32))
    cr, ci, E = out
    with np.errstate(all="ignore"):
        q = (cr * cr + ci * ci) / (E * E)
        return np.where((cr > 0) & (E > 0) & np.isfinite(q), q, F32(0))


# ---- the stream builder ----------------------------------------------------------------------------------------------------
ALTERNATING = (np.arange(148) & 1).astype(np.uint8)


def slot_bits(rng, tx, fn, tn, bsic, fcch=True, sch=True, fill="mixed"):
    """the 148 bits of slot (fn, tn) of a C0 carrier, and what it is"""
    t3 = fn % 51
    if tn == 0 and fcch and t3 in FCCH_T3:
        return np.zeros(148, np.uint8), "fcch"
    if tn == 0 and sch and t3 in SCH_T3:
        return tx.sch_encode(np.array([fn], np.uint32), np.array([bsic], np.uint8))[0], "sch"
    kind = fill if fill != "mixed" else ("random", "dummy", "random", "alternating")[int(rng.integers(0, 4))]
    if kind == "dummy":
        return DUMMY.astype(np.uint8), kind
    if kind == "alternating":
        return ALTERNATING, kind
    return rng.integers(0, 2, 148).astype(np.uint8), "random"


def build_stream(o, tx, rng, fn0, n_frames, bsic, extra_slots=2, fcch=True, sch=True, fill="mixed", loud=1.0, keep=None):
    """The clean stream (complex128) of frames [fn0, fn0 + n_frames) plus extra_slots slots, and its slots
    [(fn, tn, kind, first sample)].  loud: the amplitude of every slot that is neither FCCH nor SCH.  keep: the stream's frames
    (0 = fn0) whose TN 0 may carry FCCH / SCH (None: all); the others carry fill."""
    parts, slots, at = [], [], 0
    total = 8 * n_frames + extra_slots
    for s in range(total):
        fn, tn = (fn0 + s // 8) % HYPER, s % 8
        sync = keep is None or s // 8 in keep
        bits, kind = slot_bits(rng, tx, fn, tn, bsic, fcch and sync, sch and sync, fill)
        w = o.modulate(bits.astype(np.int8), 8 + (tn % 4 == 0)).astype(np.complex128)
        if kind not in ("fcch", "sch"):
            w = w * loud
        parts.append(w)
        slots.append((fn, tn, kind, at))
        at += len(w)
    return np.concatenate(parts), slots


def fractional_delay(x, d):
    """x delayed by d in [0, 1) samples: a Blackman-windowed sinc of 41 taps"""
    if d == 0:
        return x.copy()
    t = np.arange(-20, 21) - d
    h = np.sinc(t) * (0.42 + 0.5 * np.cos(np.pi * t / 21.0) + 0.08 * np.cos(2 * np.pi * t / 21.0))
    return np.convolve(x, h)[20:20 + len(x)]


def impair(x, rng, sps, cut=0, frac8=0, f=0.0, gain=1.0 + 0j, snr_db=None):
    """cut-in at sample `cut`, a delay of frac8 / 8 sample, a rotation by f cycles / symbol, a complex gain, Gaussian noise at
    snr_db below the nominal slot power |gain|^2.  A feature at clean sample p lands at p - cut + frac8 / 8.  -> complex64"""
    y = fractional_delay(x, frac8 / 8.0)[cut:]
    n = np.arange(len(y))
    y = y * np.exp(2j * np.pi * f * n / sps) * gain
    if snr_db is not None:
        sigma = abs(gain) * 10.0 ** (-snr_db / 20.0)
        y = y + sigma * np.sqrt(0.5) * (rng.standard_normal(len(y)) + 1j * rng.standard_normal(len(y)))
    return y.astype(np.complex64)


def first(slots, kind, after=0):
    """(fn, first sample) of the first slot of a kind that starts at or after clean sample `after`"""
    for fn, tn, k, at in slots:
        if k == kind and at >= after:
            return fn, at
    return None


# ---- the cases the CPU and the GPU tests share -------------------------------------------------------------------------------
N_FRAMES = 12                                                  # plus two slots: an FCCH and the SCH behind it always fit
# first frames: every FCCH position of the 51-multiframe, the idle frame, large T1, and two streams across the hyperframe's end.
# None puts an FCCH into the two extra slots (its SCH would lie outside the stream).
TRUTH_FN0 = (0, 10, 51 * 7 + 20, 1326 * 100 + 30, 1326 * 2047 + 51 * 3 + 40, HYPER - 5, HYPER - 11, 50, 9, 51 * 1000 + 19, 29, 38,
             45, 5, 51 * 26 * 3, 1326 * 1024 + 10)


def truth_cases(sps):
    """16 seeded cases at SNR 20 dB, |f| <= 0.1 cycle / symbol: [dict(seed, fn0, bsic, cut, frac8, f, gain)]"""
    rng = np.random.default_rng(1000 + sps)
    cases = []
    for i, fn0 in enumerate(TRUTH_FN0):
        f = (0.1, -0.1, 0.0)[i] if i < 3 else float(rng.uniform(-0.1, 0.1))
        cases.append(dict(seed=100 * sps + i, fn0=fn0, bsic=int(rng.integers(0, 64)), cut=int(rng.integers(0, 1250 * sps)),
                          frac8=int(rng.integers(0, 8)), f=f,
                          gain=complex(rng.uniform(0.3, 3.0) * np.exp(2j * np.pi * rng.uniform()))))
    return cases


def truth_stream(o, tx, case, snr_db=20.0):
    """(x complex64, the stream's SCH slots [(fn, position in x)]); every stream is padded with zeros to the uncut length"""
    rng = np.random.default_rng(case["seed"])
    clean, slots = build_stream(o, tx, rng, case["fn0"], N_FRAMES, case["bsic"])
    x = impair(clean, rng, o.sps, case["cut"], case["frac8"], case["f"], case["gain"], snr_db)
    x = np.concatenate([x, np.zeros(len(clean) - len(x), np.complex64)])
    sch = [(fn, at - case["cut"] + case["frac8"] / 8.0) for fn, tn, kind, at in slots if kind == "sch"]
    return x, sch


def negative_streams(o, tx, sps):
    """[(name, x, what must hold)]: 'no_fcch': bit 1 clear; 'no_sch': bits 1 and 2 set, bit 4 clear; 'cut': bit 1 set, 2 clear"""
    out = []
    for i, f in enumerate((0.0, 0.1, -0.1)):
        rng = np.random.default_rng(7000 + 10 * sps + i)
        clean, _ = build_stream(o, tx, rng, 3, 4, 5, fcch=False, sch=False)
        out.append(("no_fcch", impair(clean, rng, sps, int(rng.integers(0, 100)), i, f, 1.0, 20.0)))
    rng = np.random.default_rng(7100 + sps)
    clean, _ = build_stream(o, tx, rng, 10, 3, 5, sch=False, fill="random")
    out.append(("no_sch", impair(clean, rng, sps, 17, 3, 0.03, 0.8 - 0.3j, 20.0)))
    rng = np.random.default_rng(7200 + sps)
    clean, slots = build_stream(o, tx, rng, 10, 2, 5)
    x = impair(clean, rng, sps, 5, 1, -0.05, 1.0, 20.0)
    end = first(slots, "sch")[1] - 5 + 100 * sps                # the stream ends 100 symbols into the SCH burst
    out.append(("cut", x[:end]))
    return out
