"""Two-antenna burst families for the diversity equaliser's tests (tests/test_mlse_div_model.py, tests/test_gpu_mlse_div*.py): one
transmitted burst through an independent channel per antenna (mlse_family.channel, or Rayleigh taps with equal noise power),
amplitude and TOA from the oracle's analyzeTrafficBurst on each antenna and mlse_div_model.select between them.  Test INPUT
generation only; the expected values come from tests/mlse_div_model.py.  Computed once, shared; nobody writes to them."""
import functools

import numpy as np

import mlse_div_model
import mlse_family
import oraclebind
import synth

FALLBACK_AMP, FALLBACK_TOA = np.complex64(800 - 300j), np.float32(0.0)


def analyse(o, x, tsc):
    """(detected, amp, toa) of one antenna's burst."""
    r = o.analyze_traffic(x, tsc)
    good = bool(r["ok"]) and r["amp"] != 0
    return good, (np.complex64(r["amp"]) if good else FALLBACK_AMP), (np.float32(r["toa"]) if good else FALLBACK_TOA)


def choose(o, x0, x1, tsc):
    """(sel, amp, toa): select()'s antenna and its amp / TOA; neither detected counts as antenna 0 with the fallback values."""
    v0, a0, t0 = analyse(o, x0, tsc)
    v1, a1, t1 = analyse(o, x1, tsc)
    sel = int(mlse_div_model.select([v0], [a0], [v1], [a1])[0])
    return (1, a1, t1) if sel == 1 else (0, a0, t0)


def finish(o, sps, tsc, bits, xs0, xs1, amp, toa, primary, gaps0, gaps1, extra=None, enable=None):
    x0, off0, length = mlse_family.pack(xs0, gaps=gaps0)
    x1, off1, _ = mlse_family.pack(xs1, gaps=gaps1)
    amp = np.array(amp, np.complex64); toa = np.array(toa, np.float32); primary = np.array(primary, np.uint8)
    want = mlse_div_model.mlse_div_batch(sps, x0, off0, x1, off1, length, tsc, amp, toa, primary=primary, enable=enable, oracle=o)
    f = dict(sps=sps, tsc=tsc, bits=bits, x0=x0, off0=off0, x1=x1, off1=off1, length=length, amp=amp, toa=toa, primary=primary, want=want)
    f.update(extra or {})
    return f


KINDS = [("flat", None), ("flat", 12.0), ("five", 15.0), ("precursor", 15.0), ("five", None), ("precursor", 8.0)]


@functools.lru_cache(maxsize=None)
def mixed_batch(sps, tsc, B, seed):
    """B bursts for the parity tests, as mlse_family.mixed_batch makes them, on two antennas: burst b's antenna 0 is of kind b % 6,
    its antenna 1 of kind (b + 2) % 6, independent tap phases and noise; 157- and 156-symbol lengths; gaps of 1 or 2 samples that
    differ between the antennas, so that the two offsets of a burst have equal parity on some bursts and different parity on others;
    every fifth TOA moved by up to three symbols off the 1/512 grid."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(sps)
    bits = synth.normal_bits(rng, B, tsc)
    xs0, xs1, amp, toa, primary = [], [], [], [], []
    for b in range(B):
        s = o.modulate(bits[b].astype(np.int8), 9 if b % 4 == 0 else 8)
        k0, k1 = KINDS[b % 6], KINDS[(b + 2) % 6]
        x0 = mlse_family.channel(rng, s, sps, mlse_family.PROFILES[k0[0]], k0[1])
        x1 = mlse_family.channel(rng, s, sps, mlse_family.PROFILES[k1[0]], k1[1])
        p, a, t = choose(o, x0, x1, tsc)
        if b % 5 == 4:
            t = np.float32(t + rng.uniform(-3.0 * sps, 3.0 * sps))
        xs0.append(x0); xs1.append(x1); amp.append(a); toa.append(t); primary.append(p)
    gaps0 = [1 if b % 3 == 0 else 2 for b in range(B)]
    gaps1 = [2 if b % 4 == 1 else 1 for b in range(B)]
    f = finish(o, sps, tsc, bits, xs0, xs1, amp, toa, primary, gaps0, gaps1)
    par = (f["off0"] % 2) * 2 + f["off1"] % 2
    assert B < 4 or len(set(par.tolist())) >= 3                # equal and different parities, wide and narrow loads on either antenna
    return f


SNRS = (None, 15.0, 8.0)
GRADED_PROFILES = ("five", "precursor", "flat")


@functools.lru_cache(maxsize=None)
def graded_batch(sps, tsc=5, per=24, seed=9100):
    """The family the float64 reference grades: 3 noise levels x `per` bursts, the profiles in turn, an independent channel (random tap
    phases, own noise) per antenna.  snr [B] (NaN = no noise) and group [B] name each burst."""
    rng = np.random.default_rng(seed + sps)
    o = oraclebind.Oracle(sps)
    B = per * len(SNRS)
    bits = synth.normal_bits(rng, B, tsc)
    xs0, xs1, amp, toa, primary, snr, group = [], [], [], [], [], [], []
    for b in range(B):
        level = SNRS[b % len(SNRS)]
        p0 = GRADED_PROFILES[(b // len(SNRS)) % 3]; p1 = GRADED_PROFILES[(b // len(SNRS) + b // (3 * len(SNRS))) % 3]
        s = o.modulate(bits[b].astype(np.int8), 9 if b % 4 == 0 else 8)
        x0 = mlse_family.channel(rng, s, sps, mlse_family.PROFILES[p0], level)
        x1 = mlse_family.channel(rng, s, sps, mlse_family.PROFILES[p1], level)
        p, a, t = choose(o, x0, x1, tsc)
        xs0.append(x0); xs1.append(x1); amp.append(a); toa.append(t); primary.append(p)
        snr.append(np.nan if level is None else level); group.append("%s + %s" % (p0, p1))
    return finish(o, sps, tsc, bits, xs0, xs1, amp, toa, primary, [1 if b % 2 == 0 else 2 for b in range(B)], [2] * B,
                  extra=dict(snr=np.array(snr), group=np.array(group)))


def rayleigh(rng, s, sps, profile, sigma, scale=1000.0):
    """s through taps profile[k] * CN(0, 1) a symbol apart, plus white noise of standard deviation sigma * scale per sample (the same
    on every antenna, whatever its fade)."""
    taps = np.asarray(profile, np.complex128)
    h = taps * (rng.standard_normal(len(taps)) + 1j * rng.standard_normal(len(taps))) / np.sqrt(2.0)
    y = np.zeros(len(s) + sps * len(h), np.complex128)
    for k, hk in enumerate(h):
        y[k * sps:k * sps + len(s)] += hk * s
    y = y[:len(s)] * scale
    y = y + sigma * scale * (rng.standard_normal(len(y)) + 1j * rng.standard_normal(len(y))) / np.sqrt(2.0)
    return y.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def rayleigh_family(sps, snr_db, n, seed, tsc=2):
    """n bursts of the "five" profile with independent Rayleigh taps per antenna and burst at one MEAN snr (equal noise power on the
    antennas): dict(o, bits, xs0, xs1, v [n, 2], amp [n, 2], toa [n, 2], sel [n])."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(sps)
    prof = np.asarray(mlse_family.PROFILES["five"], np.complex128)
    sigma = np.sqrt(np.sum(np.abs(prof) ** 2)) * 10.0 ** (-snr_db / 20.0)
    bits = synth.normal_bits(rng, n, tsc)
    xs0, xs1 = [], []
    v = np.zeros((n, 2), bool); amp = np.zeros((n, 2), np.complex64); toa = np.zeros((n, 2), np.float32)
    for b in range(n):
        s = o.modulate(bits[b].astype(np.int8), 8)
        xs0.append(rayleigh(rng, s, sps, prof, sigma)); xs1.append(rayleigh(rng, s, sps, prof, sigma))
        for a, x in enumerate((xs0[-1], xs1[-1])):
            v[b, a], amp[b, a], toa[b, a] = analyse(o, x, tsc)
    sel = mlse_div_model.select(v[:, 0], amp[:, 0], v[:, 1], amp[:, 1])
    return dict(o=o, sps=sps, tsc=tsc, bits=bits, xs0=xs0, xs1=xs1, v=v, amp=amp, toa=toa, sel=sel)
