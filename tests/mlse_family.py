"""Burst families for the sequence equaliser's tests (tests/test_mlse_model.py, tests/test_gpu_mlse*.py): the oracle's modulator,
static symbol-spaced multipath with random tap phases, white noise, the oracle's analyzeTrafficBurst for amplitude and TOA.
Test INPUT generation only; the expected values come from tests/mlse_model.py."""
import functools

import numpy as np

import mlse_model
import oraclebind
import synth

PROFILES = {                                                   # taps a symbol apart
    "flat": [1.0],
    "five": [0.7, 0.5j, -0.4, 0.3, 0.0],
    "precursor": [0.5, 0.0, 1.0, 0.4j],
}
PAYLOAD = np.r_[3:61, 87:145]                                  # bits 3..59, 88..144 and the stealing flags 60, 87


def channel(rng, s, sps, taps, snr_db, scale=1000.0):
    """s through the static channel `taps` (random phase per tap) plus white noise snr_db below the received power (None: none)."""
    h = np.asarray(taps, np.complex128) * np.exp(2j * np.pi * rng.uniform(size=len(taps)))
    y = np.zeros(len(s) + sps * len(taps), np.complex128)
    for k, hk in enumerate(h):
        y[k * sps:k * sps + len(s)] += hk * s
    y = y[:len(s)] * scale
    if snr_db is not None:
        sig = scale * np.sqrt(np.sum(np.abs(h) ** 2)) * 10.0 ** (-snr_db / 20.0)
        y = y + sig * (rng.standard_normal(len(y)) + 1j * rng.standard_normal(len(y))) / np.sqrt(2.0)
    return y.astype(np.complex64)


def pack(xs, gaps=None):
    """Bursts one after the other, gaps[b] samples of padding in front of burst b: (x, off, length)."""
    gaps = np.zeros(len(xs), np.int64) if gaps is None else np.asarray(gaps, np.int64)
    length = np.array([len(v) for v in xs], np.int32)
    off = (np.cumsum(gaps + np.r_[0, length[:-1]])).astype(np.int32)
    x = np.zeros(int(off[-1] + length[-1]) + 8, np.complex64)
    for o, v in zip(off, xs):
        x[o:o + len(v)] = v
    return x, off, length


def static_family(sps, profile, snr_db, n, seed, tsc=2):
    """n bursts of one profile: (oracle, bits [n, 148], list of bursts, amp [n], toa [n], detected [n])."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(sps)
    bits = synth.normal_bits(rng, n, tsc)
    xs, amp, toa, ok = [], [], [], []
    for b in range(n):
        x = channel(rng, o.modulate(bits[b].astype(np.int8), 8), sps, PROFILES[profile], snr_db)
        r = o.analyze_traffic(x, tsc)
        xs.append(x); amp.append(r["amp"]); toa.append(r["toa"]); ok.append(r["ok"])
    return o, bits, xs, np.array(amp, np.complex64), np.array(toa, np.float32), np.array(ok, bool)


@functools.lru_cache(maxsize=None)
def mixed_batch(sps, tsc, B, seed):
    """B bursts for the parity tests: clean, noisy and multipath bursts in turn, 157- and 156-symbol lengths, every third burst at
    an odd sample offset, amplitude and TOA from analyzeTrafficBurst with every fifth TOA moved by up to three symbols off the
    1/512 grid.  Returns a dict with the packed batch and the model's results (computed once, shared)."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(sps)
    bits = synth.normal_bits(rng, B, tsc)
    kinds = [("flat", None), ("flat", 12.0), ("five", 15.0), ("precursor", 15.0), ("five", None), ("precursor", 8.0)]
    xs, amp, toa = [], [], []
    for b in range(B):
        prof, snr = kinds[b % len(kinds)]
        x = channel(rng, o.modulate(bits[b].astype(np.int8), 9 if b % 4 == 0 else 8), sps, PROFILES[prof], snr)
        r = o.analyze_traffic(x, tsc)
        a, t = (r["amp"], r["toa"]) if r["ok"] and r["amp"] != 0 else (np.complex64(800 - 300j), np.float32(0.0))
        if b % 5 == 4:
            t = np.float32(t + rng.uniform(-3.0 * sps, 3.0 * sps))
        xs.append(x); amp.append(a); toa.append(t)
    x, off, length = pack(xs, gaps=[1 if b % 3 == 0 else 2 for b in range(B)])
    amp = np.array(amp, np.complex64); toa = np.array(toa, np.float32)
    want = mlse_model.mlse_batch(sps, x, off, length, tsc, amp, toa, oracle=o)
    return dict(sps=sps, tsc=tsc, bits=bits, x=x, off=off, length=length, amp=amp, toa=toa, want=want)


@functools.lru_cache(maxsize=None)
def hostile_batch(sps, tsc=5, seed=99):
    """The bursts that must fall back or be skipped, between ordinary ones: all-zero samples, a NaN sample, a component of 2^31,
    147 symbols, a tiny caller-supplied amplitude, d_enable == 0.  `kind` names each burst."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(sps)
    kind = ["plain", "zeros", "nan", "plain", "big", "short", "tiny_amp", "disabled", "inf", "plain"]
    B = len(kind)
    bits = synth.normal_bits(rng, B, tsc)
    xs, amp, toa = [], [], []
    for b, k in enumerate(kind):
        x = channel(rng, o.modulate(bits[b].astype(np.int8), 8), sps, PROFILES["five"], 20.0)
        r = o.analyze_traffic(x, tsc)
        a, t = (r["amp"], r["toa"]) if r["ok"] and r["amp"] != 0 else (np.complex64(800 - 300j), np.float32(0.0))
        if k == "zeros":
            x[:] = 0
        elif k == "nan":
            x[70 * sps + 1:71 * sps + 1] = np.complex64(complex(np.nan, 1.0))      # (sps samples in a row: one of them is a decimated instant)
        elif k == "big":
            x[90 * sps:91 * sps] = np.complex64(complex(1.0, 2.0 ** 31) * a)
        elif k == "inf":
            x[30 * sps:31 * sps] = np.complex64(complex(-np.inf, 0.0))
        elif k == "short":
            x = x[:147 * sps]
        elif k == "tiny_amp":
            a = np.complex64(1e-12 + 1e-12j)
        xs.append(x); amp.append(a); toa.append(t)
    x, off, length = pack(xs)
    amp = np.array(amp, np.complex64); toa = np.array(toa, np.float32)
    enable = np.array([k != "disabled" for k in kind], np.uint8)
    want = mlse_model.mlse_batch(sps, x, off, length, tsc, amp, toa, enable=enable, oracle=o)
    return dict(sps=sps, tsc=tsc, kind=kind, bits=bits, x=x, off=off, length=length, amp=amp, toa=toa, enable=enable, want=want)
