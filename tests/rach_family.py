"""An adversarial family of access bursts for detectRACHBurst's certified shortcuts (csrc/trxsig_rach.hip), and the classifier
that says -- from the CPU oracle alone -- what each member is.  CPU only: no native library is loaded here.

The device detector steers with an approximate correlation and recomputes exactly only where it has to: the 26 lags round the
approximate argmax and the "far contenders" (lags whose approximate power is within RACH_DELTA = 4e-3, or the 2 D amplitude
bar, of the approximate maximum).  0..6 far contenders: two bursts of a workgroup share the exact pass; 7..38: the wave works
alone; more, or no maximum: exact at every lag; an exact argmax that leaves Ma +- 1: the neighbourhood is recomputed; a valley
sum rach_decide cannot judge: the hand-over list.  Random bursts reach almost none of that, so every class below is built to
sit on one of those branches:

  far_tie       two copies 20 / 40 / 80 symbols apart whose exact float32 peak powers tie (the second copy's amplitude bisected
                in float64), swept in 13 steps of 3e-8 across the flip of the reference's argmax
  near_tie      two copies 2 / 5 / 9 / 12 samples apart, bisected the same way: the two largest powers tie INSIDE the
                neighbourhood, 2..12 lags apart (the exact argmax leaves Ma +- 1)
  half_sample   one copy whose fractional delay is bisected so that |corr[M]|^2 ~ |corr[M+1]|^2, swept across the flip
  contend_k     K equalised copies: K - 1 far contenders in {1, 2, 6, 7, 8} (both sides of the pairing limit of 6), and designed
                correlations with 37 / 38 far contenders (this side of the limit of 38)
  contend_many  white noise, and sums of many weak copies of the synch sequence designed to 39 .. 60 far contenders
  edge_early    advanced so that the argmax is in 0..11 (0 included)
  edge_late     delayed: argmax in N-12 .. N-2, truncated valleys (2 <= numSamples < full), numSamples < 2, and full valleys
  flat          silence, a constant, a tone, one impulse, the synch sequence alone
  scale         ordinary bursts x 1e-18 and x 1e12
  ragged        lengths one below / above each limit of include/trxsig.h (in samples and in symbols), a short legal length, an
                odd sample offset, a negative offset
contend_k and edge_* members come a second and third time with noise (sigma 0.05 and 0.3 of the amplitude) added after
construction; those copies are classified again like everything else and keep their class label only if they still satisfy it
(otherwise: "noisy").

The classifier's far contenders are the lags within 2e-3 (half of RACH_DELTA; the steering error is <= 1.2e-5 of the maximum)
of the exact maximum outside [argmax - 13, argmax + 12]: a lag that passes is certainly a contender in the kernel.

Helper module, no tests here (tests/test_rach_family.py holds the census, tests/test_gpu_rach_family.py grades the kernels).
"""
import functools
import os
import re

import numpy as np

import oraclebind
import synth
from oraclebind import NO_DELAY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240
NEAR = 2e-3                 # half of RACH_DELTA (csrc/trxsig_rach.hip)
NB_LO, NB_HI = 13, 12       # the neighbourhood [argmax - 13, argmax + 12] the kernel always recomputes
PAIR_LIMIT, ALONE_LIMIT = 6, 38
AMP = 1000.0
CLASSES = ("far_tie", "near_tie", "half_sample", "contend_k", "contend_many", "edge_early", "edge_late", "flat", "scale",
           "ragged")


def length_limits():
    """(lo, hi): lo*sps <= length <= hi*sps, read from the library's header."""
    with open(os.path.join(ROOT, "include", "trxsig.h")) as f:
        m = re.search(r"(\d+)\*sps\s*<=\s*length\[b\]\s*<=\s*(\d+)\*sps", f.read())
    assert m, "include/trxsig.h no longer states the accepted burst lengths"
    return int(m.group(1)), int(m.group(2))


def accepted(sps, off, length):
    lo, hi = length_limits()
    off = np.asarray(off); length = np.asarray(length)
    return (off >= 0) & (length >= lo * sps) & (length <= hi * sps) & (length % sps == 0)


@functools.lru_cache(maxsize=None)
def oracle(sps):
    return oraclebind.Oracle(sps)


def power32(c):
    """|.|^2 as the reference forms it in float32 (Complex.h norm2: two rounded products, one rounded sum)."""
    c = np.asarray(c, np.complex64)
    r, i = c.real.astype(np.float32), c.imag.astype(np.float32)
    return i * i + r * r


def corr_power(sps, x):
    """float32 powers of detectRACHBurst's correlation, every lag."""
    o = oracle(sps)
    return power32(o.correlate(np.asarray(x, np.complex64), o.rach, NO_DELAY))


def classify(sps, x):
    """The facts of one accepted burst, from the oracle alone."""
    o = oracle(sps)
    x = np.ascontiguousarray(x, np.complex64)
    n = len(x)
    c = o.correlate(x, o.rach, NO_DELAY)
    p = power32(c)
    d = o.detect_rach(x)
    f = dict(n=n, argmax=-1, far=[], top2_gap=None, top2_dist=None, num_samples=-1, full=50 * sps + 1,
             peak_to_mean=float(d["peak_to_mean"]), ok=d["ok"], amp=d["amp"], toa=float(d["toa"]),
             finite=bool(np.isfinite(p).all() and np.isfinite(d["toa"]) and np.isfinite(d["peak_to_mean"])
                         and np.isfinite(d["amp"].real) and np.isfinite(d["amp"].imag)))
    if not (p > 0).any():
        return f
    M = int(np.argmax(p))                                      # first maximum (peakDetect: strict >)
    pm = float(p[M])
    f["argmax"] = M
    lag = np.arange(n)
    outside = (lag < M - NB_LO) | (lag > M + NB_HI)
    f["far"] = [int(t) for t in np.flatnonzero(outside & (p.astype(np.float64) >= pm * (1.0 - NEAR)))]
    f["far_loose"] = int((outside & (p.astype(np.float64) >= pm * (1.0 - 2e-2))).sum())
    order = np.argsort(-p.astype(np.float64), kind="stable")
    f["top2_gap"] = (pm - float(p[order[1]])) / pm
    f["top2_dist"] = abs(int(order[1]) - M)
    f["second"] = int(order[1])
    _, ix, _ = o.peak_detect(c)
    if ix >= 0.0 and not ix > np.float32(n):
        pk = int(np.rint(ix))
        f["num_samples"] = int(sum(1 for i in range(57 * sps, 107 * sps + 1) if pk + i < n))
    return f


# ---- building blocks ---------------------------------------------------------------------------------
def _clean(sps, rng):
    """One unit-amplitude access burst, 157 symbols, complex128."""
    return synth.modulate(synth.rach_bits(rng, 1), sps)[0].astype(np.complex128)


def _place(base, d, n):
    """base delayed by d samples (any sign, fractional part by a 21-tap sinc) in a window of n samples."""
    di = int(np.floor(d)); fr = float(d - di)
    y = base
    if fr != 0.0:
        taps = np.sinc(np.arange(21) - 10 - fr)
        y = np.convolve(base, taps)[10:10 + len(base)]         # y[t] = sum_j taps[j] base[t + 10 - j]
    out = np.zeros(n, np.complex128)
    lo, hi = max(0, di), min(n, di + len(y))
    if hi > lo:
        out[lo:hi] = y[lo - di:hi - di]
    return out


def _c64(x):
    return np.asarray(x).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def peak0(sps):
    """The correlation peak's lag for a clean burst at delay 0."""
    return int(np.argmax(corr_power(sps, _c64(AMP * _clean(sps, np.random.default_rng(1))))))


@functools.lru_cache(maxsize=None)
def centre(sps):
    """The fractional delay that puts a clean burst's interpolated correlation peak ON lag peak0 (at delay 0 it lies up to half
    a sample off, and a neighbour's sidelobe can then move the maximum to the next lag)."""
    o = oracle(sps)
    x = _c64(AMP * _clean(sps, np.random.default_rng(1)))
    _, ix, _ = o.peak_detect(o.correlate(x, o.rach, NO_DELAY))
    return float(peak0(sps) - ix)


def _bisect(build, f, lo, hi, steps=60):
    """r with f(build(r)) changing sign between lo and hi (float64 bisection; f is evaluated on the float32 burst)."""
    slo = f(build(lo)) > 0
    assert (f(build(hi)) > 0) != slo, "the bracket does not contain the flip"
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        if (f(build(mid)) > 0) == slo:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _far_tie(sps, rng, sym_apart):
    n = 157 * sps
    a = AMP * np.exp(2j * np.pi * rng.uniform())
    c1 = _place(_clean(sps, rng), 0, n)
    c2 = _place(_clean(sps, rng), sym_apart * sps, n) * np.exp(2j * np.pi * rng.uniform())
    l1 = peak0(sps); l2 = l1 + sym_apart * sps
    build = lambda r: _c64(a * (c1 + r * c2))

    def f(x):
        p = corr_power(sps, x)
        return float(p[l2]) - float(p[l1])
    r0 = _bisect(build, f, 0.5, 2.0)
    return [build(r0 * (1.0 + 3e-8 * k)) for k in range(-6, 7)], (l1, l2)


def _near_tie(sps, rng, apart):
    """Two copies `apart` samples apart; the relative phase is the first of a few that leaves the two largest powers 2..12 lags
    apart once the amplitudes are bisected to a tie."""
    n = 157 * sps
    a = AMP * np.exp(2j * np.pi * rng.uniform())
    b1 = _clean(sps, rng)                                       # the same payload twice: the two peaks have the same shape
    c1 = _place(b1, 0, n); l1 = peak0(sps)
    for ph in (0.5, 1.0, 0.75, 0.25, 0.0):
        c2 = _place(b1, apart, n) * np.exp(1j * np.pi * ph)
        build = lambda r: _c64(a * (c1 + r * c2))
        w0, w1 = l1 - 3 * sps - 2, l1 + apart + 3 * sps + 3

        def f(x):
            p = corr_power(sps, x)[w0:w1].astype(np.float64)
            top = np.flatnonzero((p[1:-1] > p[:-2]) & (p[1:-1] >= p[2:])) + 1      # local maxima
            top = top[np.argsort(-p[top], kind="stable")][:2]
            if len(top) < 2 or p[top[1]] < 0.5 * p[top[0]]:    # one peak only: which side of the middle it is on
                return 1.0 if w0 + top[0] > l1 + 0.5 * apart else -1.0
            return p[top.max()] - p[top.min()]                  # later minus earlier of the two leading peaks
        try:
            r0 = _bisect(build, f, 0.4, 2.5)
        except AssertionError:
            continue
        out = [build(r0 * (1.0 + 3e-8 * k)) for k in range(-2, 3)]
        fs = [classify(sps, x) for x in out]
        if sum(1 for q in fs if q["top2_gap"] <= 1e-6 and 2 <= q["top2_dist"] <= 12) >= 3:
            return out
    return []


def _half_sample(sps, rng):
    n = 157 * sps
    a = AMP * np.exp(2j * np.pi * rng.uniform())
    base = _clean(sps, rng)
    M = peak0(sps)
    build = lambda fr: _c64(a * _place(base, fr, n))

    def f(x):
        p = corr_power(sps, x)
        return float(p[M + 1]) - float(p[M])
    fr0 = _bisect(build, f, 0.15, 0.85)
    return [build(fr0 + 4e-8 * k) for k in range(-6, 7)], M


def _equalised(sps, rng, K, n):
    """K copies at whole-symbol delays whose exact peak powers are equalised (40 rounds of a *= sqrt(mean / peak))."""
    spacing = 30 if 30 * (K - 1) + 50 <= 157 else 15
    l = peak0(sps) + spacing * sps * np.arange(K)
    cs = [_place(_clean(sps, rng), centre(sps) + spacing * sps * k, n) * np.exp(2j * np.pi * rng.uniform()) for k in range(K)]
    a = np.ones(K)
    amp = AMP * np.exp(2j * np.pi * rng.uniform())
    for _ in range(40):
        x = _c64(amp * sum(ak * c for ak, c in zip(a, cs)))
        pw = corr_power(sps, x).astype(np.float64)
        p = np.array([pw[t - sps:t + sps + 1].max() for t in l])   # (a neighbour's sidelobes may move a peak by a lag)
        a = a * np.sqrt(p.mean() / p)
    return _c64(amp * sum(ak * c for ak, c in zip(a, cs)))


@functools.lru_cache(maxsize=None)
def _corr_matrix(sps, n):
    """T with corr = T x: corr[t] = sum_m x[t - F + m] conj(rach[m]), F = LB / 2 (float64 model of the reference's correlation:
    for DESIGNING bursts only, every fact is then taken from the oracle)."""
    b = oracle(sps).rach.astype(np.complex128)
    LB = len(b); F = LB // 2
    T = np.zeros((n, n), np.complex128)
    for t in range(n):
        lo, hi = max(0, t - F), min(n, t - F + LB)
        T[t, lo:hi] = np.conj(b[lo - (t - F):hi - (t - F)])
    return T


@functools.lru_cache(maxsize=None)
def _corr_pinv(sps, n):
    return np.linalg.pinv(_corr_matrix(sps, n), rcond=1e-4)


def _designed(sps, rng, nfar, n, spacing_sym=3, noise=0.0):
    """A burst DESIGNED to a correlation profile (in effect a sum of many weak copies of the synch sequence, one per lag): the
    magnitude is 1 + 5e-4 at lag M (the argmax), 1 at `nfar` lags at least 14 symbols from it and 0.05 .. 0.25 at every other
    symbol-spaced lag, with random phases; between the symbol-spaced lags the profile is their raised-cosine interpolation, so
    that it stays inside the sequence's band.  Least squares first, then minimum-norm corrections that put the nfar + 1
    contending lags on their magnitudes exactly.  With `noise`, white noise at that fraction of the peaks' correlation is
    added before the corrections."""
    T = _corr_matrix(sps, n)
    ph = int(rng.integers(0, sps))
    lags = np.arange(ph, n, sps)                                # one per symbol
    jM = -(-14 // sps)                                          # M's neighbourhood [M - 13, M + 12] starts at lag >= 0
    far = jM + jM + spacing_sym * np.arange(nfar)               # ... and holds none of the contenders
    assert far[-1] < len(lags) - 1, "the window does not hold that many contenders"
    d = rng.uniform(0.05, 0.25, len(lags)) * np.exp(2j * np.pi * rng.uniform(size=len(lags)))
    d[far] = np.exp(2j * np.pi * rng.uniform(size=nfar))
    d[jM] = (1.0 + 5e-4) * np.exp(2j * np.pi * rng.uniform())
    tau = (np.arange(n)[:, None] - lags[None, :]) / float(sps)
    beta = 0.35
    den = 1.0 - (2.0 * beta * tau) ** 2
    g = np.sinc(tau) * np.cos(np.pi * beta * tau) / np.where(np.abs(den) < 1e-9, 1.0, den)
    x = _corr_pinv(sps, n) @ (g @ d)
    if noise > 0.0:
        w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        x = x + w * (noise / np.abs(T @ w).max())
    C = lags[np.concatenate([[jM], far])]
    mag = np.abs(d[np.concatenate([[jM], far])])
    clear = np.ones(n, bool)                                    # lags that must stay well below the contenders
    for c in C:
        clear[max(0, c - sps // 2 - 1):c + sps // 2 + 2] = False
    held = np.zeros(0, np.int64)                                # lags found too high: held at 0.5 from then on
    for _ in range(20):
        ref = T[C] @ x
        ref = ref / np.abs(ref) * mag                           # the contenders: their own phases, the designed magnitudes
        rows, want = [C, held], [ref, None]
        if sps > 1:                                             # ... and symmetric shoulders, so that the peak stays ON the lag
            rho = float(np.sinc(1.0 / sps) * np.cos(np.pi * beta / sps) / (1.0 - (2.0 * beta / sps) ** 2))
            rows += [C - 1, C + 1]; want += [rho * ref, rho * ref]
        rows = np.concatenate(rows)
        cur = T[rows] @ x
        h = cur[len(C):len(C) + len(held)]
        want[1] = h / np.abs(h) * 0.5
        want = np.concatenate(want)
        x = x + np.linalg.lstsq(T[rows], want - cur, rcond=None)[0]   # minimum-norm correction
        high = np.flatnonzero(clear & (np.abs(T @ x) > 0.8))
        if len(high) == 0:
            break
        held = np.union1d(held, high)
    return _c64(x * (AMP / np.sqrt(np.mean(np.abs(x) ** 2))))


# ---- the family ----------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, sps, seed):
        self.sps, self.rng = sps, np.random.default_rng(seed)
        self.items = []                                         # (cls, samples complex64, forced length or None, pad before)

    def n(self):
        """The length the next member gets (synth.burst_lengths: 157 symbols at index % 4 == 0, else 156)."""
        return (148 + (9 if len(self.items) % 4 == 0 else 8)) * self.sps

    def add(self, cls, x, sigma=0.0, force=None, pad=0):
        n = self.n() if force is None else force
        y = np.zeros(n, np.complex64)
        m = min(n, len(x))
        y[:m] = _c64(x)[:m]
        if sigma > 0.0:
            a = float(np.sqrt(np.mean(np.abs(y.astype(np.complex128)) ** 2))) or 1.0
            y = _c64(y + sigma * a * (self.rng.standard_normal(n) + 1j * self.rng.standard_normal(n)) / np.sqrt(2.0))
        self.items.append((cls, y, force, pad))


def _satisfies(cls, f, want=None):
    """Does a member's facts satisfy its class's right-hand column?  (want: contend_k's design value)"""
    if cls == "near_tie":
        return f["top2_gap"] is not None and f["top2_gap"] <= 1e-6 and 2 <= f["top2_dist"] <= 12
    if cls == "contend_k":
        return want is not None and len(f["far"]) == want
    if cls == "contend_many":
        return len(f["far"]) > ALONE_LIMIT
    if cls == "edge_early":
        return 0 <= f["argmax"] <= 11
    if cls == "edge_late":
        return f["argmax"] >= 0
    if cls == "scale":
        return f["finite"]
    return True


def _build(sps, seed):
    B = _Builder(sps, seed)
    rng = B.rng
    sweeps = []                                                 # (cls, first index, count, the two lags or None)
    design = {}                                                 # index -> contend_k's design value
    remake = []                                                 # (cls, want, make(n)) of members that come again with noise

    for apart in (20, 40, 80):
        xs, lags = _far_tie(sps, rng, apart)
        sweeps.append(("far_tie", len(B.items), len(xs), lags))
        for x in xs:
            B.add("far_tie", x)
    for apart in (2, 5, 9, 12):
        for x in _near_tie(sps, rng, apart):
            B.add("near_tie", x)
    xs, M = _half_sample(sps, rng)
    sweeps.append(("half_sample", len(B.items), len(xs), (M, M + 1)))
    for x in xs:
        B.add("half_sample", x)

    for K in (2, 3, 7, 8, 9):
        for rep in range(2):
            s = int(rng.integers(1 << 30))
            make = lambda n, K=K, s=s: _equalised(sps, np.random.default_rng(s), K, n)
            design[len(B.items)] = K - 1
            B.add("contend_k", make(B.n()))
            remake.append(("contend_k", K - 1, make))
    for nfar in (37, 38, 38):
        s = int(rng.integers(1 << 30))
        design[len(B.items)] = nfar
        B.add("contend_k", _designed(sps, np.random.default_rng(s), nfar, B.n()))
    for nfar, sp, noise in ((39, 3, 0.0), (39, 3, 0.3), (40, 3, 0.0), (41, 3, 0.3), (42, 3, 0.0), (52, 2, 0.0), (60, 2, 0.3),
                            (60, 2, 0.0), (42, 3, 0.3), (39, 3, 0.0)):
        B.add("contend_many", _designed(sps, rng, nfar, B.n(), spacing_sym=sp, noise=noise))
    for sc in (40.0, 1.0, 2000.0):
        n = B.n()
        B.add("contend_many", sc * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))

    p0 = peak0(sps)
    early = [-(s * sps) + fr for s in (20, 26, 27, 28) for fr in (0.0, 0.37)]
    early += [float(-(p0 - L)) for L in (0, 1, 2, 5, 11)] + [-(p0 - 0.5), -(p0 + 0.4)]
    for d in early:
        s = int(rng.integers(1 << 30))
        make = lambda n, d=d, s=s: AMP * np.exp(2j * np.pi * (s % 997) / 997.0) * _place(_clean(sps, np.random.default_rng(s)), d, n)
        B.add("edge_early", make(B.n()))
        remake.append(("edge_early", None, make))
    late = [("sym", v) for v in (5, 15, 55, 60, 65, 69, 95, 100, 110)] + [("end", j) for j in (2, 3, 4, 6, 8, 10, 12)] + \
           [("endf", 2.5), ("endf", 7.3)]
    for kind, v in late:
        s = int(rng.integers(1 << 30))

        def make(n, kind=kind, v=v, s=s):
            d = v * sps + 0.3 if kind == "sym" else float(n - p0 - v)
            return AMP * np.exp(2j * np.pi * (s % 997) / 997.0) * _place(_clean(sps, np.random.default_rng(s)), d, n)
        B.add("edge_late", make(B.n()))
        remake.append(("edge_late", None, make))

    for rep in range(2):
        n = B.n(); B.add("flat", np.zeros(n))
        n = B.n(); B.add("flat", np.full(n, (100 + 50j) * (1 + rep)))
        n = B.n(); B.add("flat", 700 * np.exp(2j * np.pi * (0.013 + 0.05 * rep) * np.arange(n)))
        n = B.n(); x = np.zeros(n, np.complex128); x[(40 + 300 * rep) % n] = 500 - 200j; B.add("flat", x)
        n = B.n(); x = np.zeros(n, np.complex128); b = oracle(sps).rach
        st = (10 + 60 * rep) * sps; x[st:st + len(b)] = AMP * b; B.add("flat", x)

    for sc in (1e-18, 1e12):
        for rep in range(4):
            n = B.n()
            d = rng.integers(0, 40) * sps + rng.uniform()
            x = AMP * np.exp(2j * np.pi * rng.uniform()) * _place(_clean(sps, rng), d, n)
            B.add("scale", sc * x, sigma=(0.0, 0.1)[rep % 2])

    lo, hi = length_limits()
    ragged = [lo * sps - 1, lo * sps + 1, hi * sps - 1, hi * sps + 1, (lo - 1) * sps, (lo + 1) * sps, (hi - 1) * sps,
              (hi + 1) * sps, lo * sps, hi * sps, (lo + 8) * sps, 120 * sps + (1 if sps > 1 else 0) * (sps - 1), 100 * sps, 130 * sps]
    for i, n in enumerate(ragged):
        d = rng.integers(0, 6) * sps + rng.uniform()
        x = AMP * np.exp(2j * np.pi * rng.uniform()) * _place(_clean(sps, rng), d, 160 * sps)
        B.add("ragged", x, force=int(n), pad=(1 if i >= len(ragged) - 2 else 0))   # the last two: an odd sample offset
    n = B.n()
    neg_index = len(B.items)
    B.add("ragged", AMP * _place(_clean(sps, rng), 3.3, n))     # gets a negative offset below

    for sigma in (0.05, 0.3):
        for cls, want, make in remake:
            if want is not None:
                design[len(B.items)] = want
            B.add(cls, make(B.n()), sigma=sigma)

    # pack
    parts, off, length, pos = [], [], [], 0
    for cls, y, force, pad in B.items:
        if pad and (pos & 1) == 0:                              # an odd sample offset was asked for
            parts.append(np.zeros(1, np.complex64)); pos += 1
        off.append(pos); length.append(len(y)); parts.append(y); pos += len(y)
    x = np.concatenate(parts)
    off = np.array(off, np.int32); length = np.array(length, np.int32)
    off[neg_index] = -2
    cls = np.array([it[0] for it in B.items], dtype=object)
    ok = accepted(sps, off, length)
    facts = [classify(sps, x[off[i]:off[i] + length[i]]) if ok[i] else None for i in range(len(off))]
    noisy_from = len(B.items) - 2 * len(remake)
    for i in range(noisy_from, len(off)):                       # the noisy copies: re-classified, not assumed
        if not _satisfies(cls[i], facts[i], design.get(i)):
            cls[i] = "noisy"
    for a in (x, off, length):
        a.setflags(write=False)
    return dict(sps=sps, x=x, off=off, length=length, cls=cls, facts=facts, accepted=ok, sweeps=sweeps, design=design,
                noisy_from=noisy_from)


@functools.lru_cache(maxsize=None)
def family_info(sps, seed=SEED):
    """Everything about the family of (sps, seed): the packed batch, labels, per-burst facts (None for a refused burst), the
    sweeps [(class, first index, count, (lag, lag))] and contend_k's design values {index: far contenders}."""
    return _build(sps, seed)


def family(sps, seed=SEED):
    """x (packed complex64), off, length (int32), cls (class label per burst).  Read-only arrays, built once per process."""
    f = family_info(sps, seed)
    return f["x"], f["off"], f["length"], f["cls"]


def satisfies(info, i):
    """Does member i satisfy its class's right-hand column (module docstring)?"""
    f = info["facts"][i]
    if f is None:
        return info["cls"][i] == "ragged"
    return _satisfies(info["cls"][i], f, info["design"].get(i))


def census(info):
    """{class: (members, members that satisfy the class's condition)}."""
    out = {}
    for c in CLASSES + ("noisy",):
        idx = [i for i in range(len(info["cls"])) if info["cls"][i] == c]
        out[c] = (len(idx), sum(1 for i in idx if satisfies(info, i)))
    return out
