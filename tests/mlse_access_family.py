"""Access-burst families for the access-burst sequence equaliser's tests (tests/test_mlse_access_model.py,
tests/test_gpu_mlse_access*.py): the oracle's modulator, tests/mlse_family.py's static multipath and noise, a random delay in
front of the burst, the oracle's detectRACHBurst for amplitude and TOA.  Test INPUT generation only; the expected values come from
tests/mlse_access_model.py."""
import functools

import numpy as np

import fecbind
import l1_ms_model as lms
import mlse_access_model as model
import mlse_family
import oraclebind

PAYLOAD = np.arange(49, 85)                                    # the 36 coded bits


@functools.lru_cache(maxsize=None)
def _fo():
    return fecbind.FecOracle()


def access_bits(rng, n, bsic=None):
    """(bits [n, 148], ra [n], bsic [n]): access bursts with random RA (and BSIC, unless one is given)."""
    ra = rng.integers(0, 256, n); bs = rng.integers(0, 64, n) if bsic is None else np.full(n, bsic)
    return np.stack([lms.access_burst(_fo(), int(r), int(b)) for r, b in zip(ra, bs)]), ra, bs


def received(rng, o, bits, sps, profile, snr_db, delay_sym, nsym=156):
    """One burst's `nsym` symbols of received samples: the burst `delay_sym` symbols (any real number) into the window, through the
    profile's channel with noise."""
    s = o.modulate(bits.astype(np.int8), 68)                  # 148 + 68 symbols: enough behind the burst for any delay
    d = int(round(delay_sym * sps))
    s = np.r_[np.zeros(d, np.complex64), s]
    x = mlse_family.channel(rng, s, sps, mlse_family.PROFILES[profile], snr_db)
    return np.ascontiguousarray(x[:nsym * sps])


def static_family(sps, profile, snr_db, n, seed, max_delay=29):
    """n bursts of one profile, each delayed by 0..max_delay whole symbols: (oracle, bits [n, 148], ra, bsic, list of bursts, amp [n],
    toa [n], detected [n]) with detectRACHBurst's default threshold."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(sps)
    bits, ra, bsic = access_bits(rng, n)
    xs, amp, toa, ok = [], [], [], []
    for b in range(n):
        x = received(rng, o, bits[b], sps, profile, snr_db, int(rng.integers(0, max_delay + 1)))
        r = o.detect_rach(x)
        xs.append(x); amp.append(r["amp"]); toa.append(r["toa"]); ok.append(r["ok"])
    return o, bits, ra, bsic, xs, np.array(amp, np.complex64), np.array(toa, np.float32), np.array(ok, bool)


@functools.lru_cache(maxsize=None)
def mixed_batch(sps, B, seed):
    """B access bursts for the parity tests: clean, noisy and multipath bursts in turn, 157- and 156-symbol lengths, every third
    burst at an odd sample offset, delays of 0..60 symbols, amplitude and TOA from detectRACHBurst (a fixed pair where it finds
    nothing) with every fifth TOA moved off the 1/512 grid.  Returns a dict with the packed batch and the model's results
    (computed once, shared)."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(sps)
    bits, ra, bsic = access_bits(rng, B)
    kinds = [("flat", None), ("flat", 12.0), ("five", 15.0), ("precursor", 15.0), ("five", None), ("precursor", 8.0)]
    xs, amp, toa = [], [], []
    for b in range(B):
        prof, snr = kinds[b % len(kinds)]
        delay = [0.0, 7.0, 29.0, 60.0, 3.25, 41.0][(b // 2) % 6]
        x = received(rng, o, bits[b], sps, prof, snr, delay, 157 if b % 4 == 0 else 156)
        r = o.detect_rach(x)
        a, t = (r["amp"], r["toa"]) if r["ok"] and r["amp"] != 0 else (np.complex64(800 - 300j), np.float32(delay * sps))
        if b % 5 == 4:
            t = np.float32(t + rng.uniform(-1.0 * sps, 1.0 * sps))
        xs.append(x); amp.append(a); toa.append(t)
    x, off, length = mlse_family.pack(xs, gaps=[1 if b % 3 == 0 else 2 for b in range(B)])
    amp = np.array(amp, np.complex64); toa = np.array(toa, np.float32)
    want = model.access_batch(sps, x, off, length, amp, toa, oracle=o)
    return dict(sps=sps, bits=bits, ra=ra, bsic=bsic, x=x, off=off, length=length, amp=amp, toa=toa, want=want)


@functools.lru_cache(maxsize=None)
def hostile_batch(sps, seed=97):
    """tests/mlse_family.py's hostile set remade for access bursts: all-zero samples, a NaN sample, a component of 2^31, an infinity,
    147 symbols, a tiny caller-supplied amplitude, d_enable == 0, between ordinary bursts.  `kind` names each burst."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(sps)
    kind = ["plain", "zeros", "nan", "plain", "big", "short", "tiny_amp", "disabled", "inf", "plain"]
    B = len(kind)
    bits, ra, bsic = access_bits(rng, B)
    xs, amp, toa = [], [], []
    for b, k in enumerate(kind):
        x = received(rng, o, bits[b], sps, "five", 20.0, 2)
        r = o.detect_rach(x)
        a, t = (r["amp"], r["toa"]) if r["ok"] and r["amp"] != 0 else (np.complex64(800 - 300j), np.float32(2 * sps))
        if k == "zeros":
            x[:] = 0
        elif k == "nan":
            x[70 * sps + 1:71 * sps + 1] = np.complex64(complex(np.nan, 1.0))      # (sps samples in a row: one of them is a decimated instant)
        elif k == "big":
            x[60 * sps:61 * sps] = np.complex64(complex(1.0, 2.0 ** 31) * a)
        elif k == "inf":
            x[30 * sps:31 * sps] = np.complex64(complex(-np.inf, 0.0))
        elif k == "short":
            x = x[:147 * sps]
        elif k == "tiny_amp":
            a = np.complex64(1e-12 + 1e-12j)
        xs.append(x); amp.append(a); toa.append(t)
    x, off, length = mlse_family.pack(xs)
    amp = np.array(amp, np.complex64); toa = np.array(toa, np.float32)
    enable = np.array([k != "disabled" for k in kind], np.uint8)
    want = model.access_batch(sps, x, off, length, amp, toa, enable=enable, oracle=o)
    return dict(sps=sps, kind=kind, bits=bits, x=x, off=off, length=length, amp=amp, toa=toa, enable=enable, want=want)
