"""An adversarial family for the equaliser (csrc/trxsig_eq_est.hip, trxsig_eq_dfe.hip: k_eq_detect in its two instantiations, k_eq_detect52,
k_eq_estimate_wave, k_design_dfe, k_eq_delay + k_eq_dfe2 and the fused k_eq_dfe4) and the one oracle chain every equaliser
test compares with.  No GPU, no torch, no native product library here; seeded, the same members everywhere.

oracle_chain(o, s, tsc, thr_or_snr, variant52m, max_toa) is the per-burst sequence of Transceiver::pullRadioVector's TSC leg
(Transceiver.cpp:326-349, 391-396) on the CPU oracle: analyzeTrafficBurst(requestChannel), 1 / amp as Complex.h forms it,
the SNR estimate in the reference's mixed float / double arithmetic, designDFE of the scaled channel and equalizeBurst of
the scaled burst at TOA - chanRespOffset.

The members, by what they are after:
  geometry(max_toa)  the 52M window for ONE maxTOA (0 .. 17: `max_toa < 3` is clamped to 3, the span is max(maxTOA, 5), and
                     startIx, corrLen and the admissible channel-pick windows all move with it, ref52:983-1000, 1053-1062):
                     131 bursts that arrive up to maxTOA + 1.5 symbols early or late, so the peak falls on every lag and past
                     both window edges; every sixth is noise x 100, one integer impulse, silence or a ragged length
                     (92 .. 156, or from the shortest burst the window fits in: ragged_floor).
  channels()         channel estimates and SNRs for designDFE alone: seven rounds of divisions and reciprocal square roots
                     (design_dfe7 / design_dfe7_lanes) on random channels, one of them scaled by 2^-70 .. 2^62, unit vectors,
                     the zero channel, h[0] = 0, the alternating channel, NaN and Inf taps, SNRs from 0 and a denormal to
                     Inf and NaN, and 1 / amp scaling with amp 0, a denormal, Inf and NaN.
  bursts()           whole bursts for the full chain in both variants: one clean burst times 2^k, k = -30 .. 53 (detection
                     holds from about 2^-28 to 2^51; an energy gate at 10 refuses the rungs below 2^-7, so the tests
                     also run it with the gate off or at 0), channels beyond one echo (five decaying echoes, a spectral null, a weak
                     first path), one NaN / +-Inf sample in four places, constant bursts.
  taps()             caller-supplied taps for trxsig_equalize_taps_batch: every length 92 .. 157, each w[j] and b[j] in turn
                     +Inf, -Inf or NaN in either part, all-NaN taps, amp 0 / Inf / NaN, silent bursts under finite taps
                     (every pre-decision value of the first symbol is an exact zero, which `> 0` sends to -1), taps of 1e30.
                     The reference SKIPS a feed-forward term beyond the burst (convolve, sigProcLib.cpp:322-366); an
                     equaliser that multiplies a zero sample instead turns the last 6 - j soft bits into NaN when w[j] is
                     not finite (equalize_member(pad=6) below is that mutant).

Helper module, no tests here: tests/test_eq_family.py proves the family, tests/test_gpu_eq_family.py grades the kernels."""
import functools

import numpy as np

import synth
from util import veq_nan

F32 = np.float32
C64 = np.complex64
MAX_TOAS = tuple(range(18))
FP16_MAX_TOAS = (0, 3, 5, 6, 17)
GEOMETRY_B = 131                                               # two workgroups of 64 lanes and three bursts
BURSTS_TSC, BURSTS_MAX_TOA = 5, 4


class Snr(float):
    """oracle_chain's thr_or_snr: the SNR estimate itself (trxsig_estimate_dfe_batch's snr_value) instead of a threshold."""


def inv_amp(amp):
    """complex(1, 0) / amp as Complex.h forms it (:85, 119, 154-160), every operation in float32: norm2 = i*i + r*r,
    inv = (r / norm2, -i / norm2), then the product with (1, 0) -- which turns (Inf, -Inf) into NaNs, as the reference does."""
    with np.errstate(all="ignore"):
        r, i = F32(np.real(amp)), F32(np.imag(amp))
        n2 = F32(F32(i * i) + F32(r * r))
        ir, ii = F32(r / n2), F32(-i / n2)
        one, zero = F32(1.0), F32(0.0)
        return complex(F32(F32(one * ir) - F32(zero * ii)), F32(F32(one * ii) + F32(zero * ir)))


def snr_estimate(amp, thr):
    """SNR = |amp|^2 / (thr^2 + 1) (Transceiver.cpp:340): norm2 and thr^2 in float32, the quotient in double, a float32 result."""
    with np.errstate(all="ignore"):
        r, i = F32(np.real(amp)), F32(np.imag(amp))
        n2 = F32(F32(i * i) + F32(r * r))
        t = F32(thr)
        return F32(np.float64(n2) / (np.float64(F32(t * t)) + 1.0))


def oracle_chain(o, s, tsc, thr_or_snr, variant52m, max_toa, analyzer=None):
    """One burst through the equalised leg on oracle `o` (oraclebind.Oracle(1, variant52m)).  thr_or_snr: the threshold that
    enters the SNR estimate (the energy threshold of trxsig_equalize_normal_batch, 0 with its gate off; snr_thresh of
    trxsig_estimate_dfe_batch) or Snr(v), the estimate itself.  Returns a dict: ok, amp, toa and -- None unless ok -- chan,
    chan_off, snr, w, b, soft.  analyzer: stands in for o.analyze_traffic (the tests' geometry mutant)."""
    assert bool(o.variant52m) == bool(variant52m)
    a = (analyzer or o.analyze_traffic)(s, tsc, 3.0, req_chan=True, max_toa=max_toa)
    r = dict(ok=a["ok"], amp=a["amp"], toa=a["toa"], chan=None, chan_off=None, snr=None, w=None, b=None, soft=None)
    if not a["ok"]:
        return r
    inv = inv_amp(a["amp"])
    snr = F32(thr_or_snr) if isinstance(thr_or_snr, Snr) else snr_estimate(a["amp"], thr_or_snr)
    w, b = o.design_dfe(o.scale_vector(a["chan"], inv), float(snr), 7)
    soft = o.equalize(o.scale_vector(s, inv), F32(a["toa"] - a["chan_off"]), w, b)
    r.update(chan=a["chan"], chan_off=a["chan_off"], snr=snr, w=w, b=b, soft=soft)
    return r


class Batch:
    """Packed bursts: x complex64 (burst i at x[off[i] : off[i] + length[i]]), and whatever labels the maker adds."""

    def __init__(self, x, off, length, **labels):
        self.x, self.off, self.length = np.ascontiguousarray(x, C64), np.ascontiguousarray(off, np.int32), \
            np.ascontiguousarray(length, np.int32)
        self.__dict__.update(labels)
        for a in (self.x, self.off, self.length):
            a.setflags(write=False)

    def __len__(self):
        return len(self.off)

    def burst(self, i):
        return self.x[self.off[i]:self.off[i] + self.length[i]]

    def take(self, rows):
        """The bursts `rows`, repacked end to end."""
        return pack([self.burst(i) for i in rows])


def pack(bursts, gaps=None, first=0):
    n = len(bursts)
    gaps = np.zeros(n, np.int64) if gaps is None else np.asarray(gaps, np.int64)
    length = np.array([len(s) for s in bursts], np.int32)
    off = (first + np.concatenate([[0], np.cumsum(length[:-1] + gaps[:-1])])).astype(np.int32)
    x = np.zeros(int(off[-1] + length[-1]) + 8, C64)
    for s, o in zip(bursts, off):
        x[o:o + len(s)] = s
    return Batch(x, off, length)


def _noise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(C64)


def fp16_exact(x):
    """x scaled so that its largest component is 2000 and rounded to integers: exact in float16 and in float32 alike."""
    v = np.ascontiguousarray(x, C64).view(F32)
    scale = 2000.0 / np.abs(v[np.isfinite(v)]).max()
    return np.clip(np.rint(v * scale), -2048, 2048).astype(F32).view(C64)


# ---- geometry ----
def ragged_floor(max_toa):
    """The shortest burst whose 52M correlation window fits: the reference reads samples 66 - span .. 81 + span unchecked
    (span = max(maxTOA, 5)), so above maxTOA 10 the ragged members cannot go down to 92.  What the library does with a
    shorter burst (F_BADLEN) is tests/test_gpu_eq_family.py's to check, with no reference to compare."""
    return max(92, 82 + max(max_toa, 5))


@functools.lru_cache(maxsize=None)
def geometry(max_toa, integers=False):
    """Bursts for the 52M window with this maxTOA; `kind`: -1 a burst, 0 noise, 1 an impulse, 2 silence, 3 a ragged length.
    integers: the same members as fp16-exact integers (both storages then hold the same numbers)."""
    B, tsc = GEOMETRY_B, (3 * max_toa + 1) % 8
    x, off, length, meta = synth.normal_batch(1, B, tsc, seed=6100 + max_toa, sigmas=(0.02, 0.3), max_delay=max_toa + 1.5)
    rng = np.random.default_rng(6200 + max_toa)
    x, length = x.copy(), length.copy()
    kind = np.full(B, -1)
    for i in range(0, B, 6):
        s = x[off[i]:off[i] + length[i]]
        kind[i] = (i // 6) % 4
        if kind[i] == 0:
            s[:] = _noise(rng, len(s)) * F32(100.0)
        elif kind[i] == 1:
            s[:] = 0
            s[int(rng.integers(40, 111))] = C64(complex(rng.integers(1, 50), rng.integers(-50, 50)))
        elif kind[i] == 2:
            s[:] = 0
        else:
            length[i] = rng.integers(ragged_floor(max_toa), 157)
    if integers:
        x = fp16_exact(x)
    return Batch(x, off, length, tsc=tsc, max_toa=max_toa, kind=kind)


# ---- channels ----
class Channels:
    """chan [n, 6] complex64, snr [n] float32, amp [n] complex64 and use_amp [n] (False: designDFE of chan as it is)."""

    def __init__(self, rows):
        self.name = [r[0] for r in rows]
        self.chan = np.array([r[1] for r in rows], C64)
        self.snr = np.array([r[2] for r in rows], F32)
        self.use_amp = np.array([r[3] is not None for r in rows])
        self.amp = np.array([1.0 if r[3] is None else r[3] for r in rows], C64)
        for a in (self.chan, self.snr, self.amp, self.use_amp):
            a.setflags(write=False)

    def __len__(self):
        return len(self.snr)

    def scaled(self, o, i):
        """Member i's channel as designDFE gets it: scaleVector(chan, 1 / amp) where an amplitude is given."""
        return o.scale_vector(self.chan[i], inv_amp(self.amp[i])) if self.use_amp[i] else self.chan[i].copy()


SNRS = (0.0, -1.0, 1e-45, 1e-38, 1e-30, 1e30, 3e38, np.inf, np.nan)


@functools.lru_cache(maxsize=None)
def channels():
    rng = np.random.default_rng(7001)
    decay = 0.6 ** np.arange(6)

    def rand():
        return ((rng.standard_normal(6) + 1j * rng.standard_normal(6)) * decay).astype(C64)
    rows = []
    base = [rand() for _ in range(5)]
    for i, h in enumerate(base):
        rows.append(("random%d" % i, h, rng.uniform(1, 200), None))
        rows.append(("random%d/amp" % i, h * C64(700 - 300j), rng.uniform(1, 200), C64(700 - 300j) * C64(rng.uniform(0.5, 2))))
    for k in range(-70, 63, 6):
        rows.append(("2^%d" % k, np.ldexp(base[0].view(F32), k).view(C64), 37.5, None))
    for k in range(6):
        rows.append(("unit%d" % k, np.eye(6, dtype=C64)[k], 37.5, None))
    rows.append(("zero", np.zeros(6, C64), 37.5, None))
    h = base[1].copy(); h[0] = 0
    rows.append(("h0=0", h, 37.5, None))
    rows.append(("alternating", np.array([1, -1, 1, -1, 1, -1], C64), 1e6, None))
    h = base[2].copy(); h[3] = complex(np.nan, 0.25)
    rows.append(("nan tap", h, 37.5, None))
    h = base[2].copy(); h[1] = complex(0.5, -np.inf)
    rows.append(("inf tap", h, 37.5, None))
    for v in SNRS:
        rows.append(("snr %r" % v, base[3], v, None))
    for a in (0.0, 1e-42 + 0j, complex(np.inf, 1.0), complex(1.0, np.nan)):
        rows.append(("amp %r" % (a,), base[4], 37.5, a))
    return Channels(rows)


# ---- bursts ----
def _through(h, s):
    """The burst through the channel h (h[0] on time, h[d] d symbols late), float32 products."""
    y = np.zeros_like(s)
    for d, g in enumerate(h):
        if g != 0:
            y[d:] += (C64(g) * s[:len(s) - d]).astype(C64)
    return y


@functools.lru_cache(maxsize=None)
def bursts():
    """`cls` names each member's class; `hostile` marks those with a non-finite sample (a neighbour's results must not move
    when they leave the batch)."""
    rng = np.random.default_rng(7100)
    n_clean = 1 + 5 + 8 + 5 + 4
    bits = synth.normal_bits(rng, n_clean, BURSTS_TSC)
    base = synth.fractional_delay(synth.modulate(bits, 1), rng.uniform(-0.9, 0.9, n_clean))

    def dress(row, n=156):
        a = rng.uniform(400, 2500) * np.exp(2j * np.pi * rng.uniform())
        return a, (base[row, :n] * C64(a)).astype(C64)

    def noisy(s, a, sigma=0.02):
        return (s + F32(sigma * abs(a) / np.sqrt(2)) * _noise(rng, len(s))).astype(C64)
    out, cls = [], []
    a, s = dress(0)
    clean = noisy(s, a)
    for k in range(-30, 54):                                    # the ladder: exact powers of two
        out.append(np.ldexp(clean.view(F32), k).view(C64)); cls.append("ladder")
    row = 1
    for _ in range(5):                                          # (plain bursts between the classes)
        a, s = dress(row, 156 + (row & 1)); row += 1
        out.append(noisy(s, a, 0.1)); cls.append("plain")
    for _ in range(8):
        a, s = dress(row); row += 1
        h = np.concatenate([[1], (rng.standard_normal(5) + 1j * rng.standard_normal(5)) * 0.35 / np.sqrt(2) * 0.8 ** np.arange(5)])
        out.append(noisy(_through(h, s), a)); cls.append("echoes")
    for d in range(1, 6):                                       # an equal-power echo: a null in the band
        a, s = dress(row); row += 1
        h = np.zeros(d + 1, complex); h[0] = 1; h[d] = np.exp(2j * np.pi * rng.uniform())
        out.append(noisy(_through(h, s), a)); cls.append("null")
    for d in range(1, 5):                                       # a weak first path: maximum phase
        a, s = dress(row); row += 1
        h = np.zeros(d + 1, complex); h[0] = 0.3; h[d] = 1
        out.append(noisy(_through(h, s), a)); cls.append("maxphase")
    a, s = dress(0)
    victim = noisy(s, a)
    for place, at in (("window", 72), ("outside", 30), ("first", 2), ("last", 153)):
        for j, v in enumerate((np.nan, np.inf, -np.inf)):
            h = victim.copy()
            h[at + j] = complex(v, h[at + j].imag) if (j + at) & 1 else complex(h[at + j].real, v)
            out.append(h); cls.append("nonfinite/" + place)
    out.append(np.full(156, 1000, C64)); cls.append("constant")
    out.append(np.full(157, 1000j, C64)); cls.append("constant")
    bt = pack(out)
    cls = np.array(cls)
    return Batch(bt.x, bt.off, bt.length, cls=cls, hostile=np.char.startswith(cls, "nonfinite"), tsc=BURSTS_TSC,
                 max_toa=BURSTS_MAX_TOA, ladder_k=np.arange(-30, 54))


# ---- taps ----
GRID_TOAS = (0.5, -1.25, 2.75, -0.001953125, 3.0)               # on the 1/512 grid; 3.0: delayVector's copy branch
BAD = (np.inf, -np.inf, np.nan)


@functools.lru_cache(maxsize=None)
def taps():
    """A Batch of integer-valued bursts (fp16-exact) at ragged odd offsets with toa, amp [n], w [n, 7], b [n, 5] and cls:
    "finite" (random finite taps: one per length at TOA 0, one per length at a grid TOA), "w" / "b" (one component of one
    tap not finite; `bad` = (tap, value index, part), `at0` marks TOA 0), "allnan", "amp", "silent", "huge"."""
    rng = np.random.default_rng(7200)
    rows = []                                                   # (cls, length, toa, amp, w, b, silent, bad)

    def rand_taps():
        w = (rng.normal(0, 0.4, 7) + 1j * rng.normal(0, 0.4, 7)).astype(C64)
        b = (rng.normal(0, 0.2, 5) + 1j * rng.normal(0, 0.2, 5)).astype(C64)
        return w, b

    def rand_amp():                                             # of the samples' own size, so the soft bits do not all saturate
        return C64(rng.uniform(800, 4000) * np.exp(2j * np.pi * rng.uniform()))
    lens = list(range(92, 158))
    for n in lens:
        rows.append(("finite", n, 0.0, rand_amp(), *rand_taps(), False, None))
    for i, n in enumerate(lens):
        rows.append(("finite", n, GRID_TOAS[i % len(GRID_TOAS)], rand_amp(), *rand_taps(), False, None))
    at = 0
    for toa0 in (True, False):
        for which, ntap in (("w", 7), ("b", 5)):
            for j in range(ntap):
                for vi, v in enumerate(BAD):
                    for part in (0, 1):
                        w, b = rand_taps()
                        t = w if which == "w" else b
                        t[j] = complex(v, t[j].imag) if part == 0 else complex(t[j].real, v)
                        n = lens[(7 * at) % len(lens)]; at += 1
                        toa = 0.0 if toa0 else GRID_TOAS[at % len(GRID_TOAS)]
                        rows.append((which, n, toa, rand_amp(), w, b, False, (j, vi, part)))
    for n in (92, 157):
        rows.append(("allnan", n, 0.0, rand_amp(), np.full(7, complex(np.nan, np.nan), C64), np.full(5, complex(np.nan, np.nan), C64), False, None))
    for a in (0.0, complex(np.inf, 0.0), complex(0.0, -np.inf), complex(np.nan, 1.0), 1e-42 + 0j):
        rows.append(("amp", 148 + len(rows) % 9, 0.5, C64(a), *rand_taps(), False, None))
    for n in (92, 120, 148, 156, 157, 133, 101, 155):
        rows.append(("silent", n, GRID_TOAS[n % len(GRID_TOAS)], rand_amp(), *rand_taps(), True, None))
    for n in (93, 156, 157, 140):
        w, b = rand_taps()
        rows.append(("huge", n, 0.0, C64(1.0), (w * C64(2.5e30)).astype(C64), (b * C64(5e30)).astype(C64), False, None))
    bs = []
    for r in rows:
        n = r[1]
        s = (rng.integers(-1500, 1501, n) + 1j * rng.integers(-1500, 1501, n)).astype(C64)
        bs.append(np.zeros(n, C64) if r[6] else s)
    bt = pack(bs, gaps=rng.integers(0, 4, len(rows)), first=1)
    cls = np.array([r[0] for r in rows])
    toa = np.array([r[2] for r in rows], F32)
    return Batch(bt.x, bt.off, bt.length, cls=cls, toa=toa, amp=np.array([r[3] for r in rows], C64),
                 w=np.array([r[4] for r in rows], C64), b=np.array([r[5] for r in rows], C64), bad=[r[7] for r in rows],
                 at0=toa == 0)


def equalize_member(o, t, i, pad=0):
    """scaleVector(burst, 1 / amp) + equalizeBurst of member i of taps() on oracle o.  pad > 0 is the ZERO-PAD MUTANT: the
    burst followed by `pad` zero samples, the output cut back to the burst's length -- an equaliser that meets zero samples
    beyond the burst where the reference skips the terms."""
    s = o.scale_vector(t.burst(i), inv_amp(t.amp[i]))
    if pad:
        s = np.concatenate([s, np.zeros(pad, C64)])
    return o.equalize(s, t.toa[i], t.w[i], t.b[i])[:t.length[i]]


def same_with_nan(a, b):
    """util.veq_nan everywhere, as a predicate."""
    return np.shape(a) == np.shape(b) and bool(veq_nan(a, b).all())


def chain_batch(o, x, off, length, tsc, detect_thresh, energy_thresh, max_toa):
    """The reference driver's eq_batch (oracle/ref_driver.cpp: energyDetect, then the chain, burst by burst) on oracle o:
    ok [B] uint8 and soft [B, 157] float32, rows of zeros where the gate or the detector said no."""
    assert detect_thresh == 3.0
    B = len(off)
    ok, soft = np.zeros(B, np.uint8), np.zeros((B, 157), F32)
    for i in range(B):
        s = x[off[i]:off[i] + length[i]]
        if not o.energy_detect(s, 20, energy_thresh)[0]:
            continue
        c = oracle_chain(o, s, tsc, energy_thresh, o.variant52m, max_toa)
        if c["ok"]:
            ok[i] = 1
            soft[i, :min(157, len(c["soft"]))] = c["soft"][:157]
    return ok, soft
