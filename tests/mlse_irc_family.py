"""Two-antenna burst families with a co-channel interferer for the interference-rejection equaliser's tests
(tests/test_mlse_irc_model.py, tests/test_gpu_mlse_irc*.py): mlse_div_family's families with a second handset's normal burst
(another training sequence, random payload) reaching both antennas through channels of its own.  Test INPUT generation only; the
expected values come from tests/mlse_irc_model.py.  Computed once, shared; nobody writes to them."""
import functools

import numpy as np

import mlse_div_family as dfam
import mlse_div_model as dm
import mlse_family
import mlse_irc_model as im
import oraclebind
import synth

INTERFERER_KINDS = [("flat", 3.0), ("five", 0.0), None, ("flat", 0.0), ("precursor", 6.0), ("five", 10.0)]      # (profile, C/I in dB)


def with_model(f, loading=im.LOADING):
    """f with want = the IRC model's results on it (the symbols of f's own diversity run are reused where f has them)."""
    y = f["want"]["y"] if "want" in f else None
    want = im.mlse_irc_batch(f["sps"], f["x0"], f["off0"], f["x1"], f["off1"], f["length"], f["tsc"], f["amp"], f["toa"], primary=f["primary"],
                             loading=loading, y=y)
    return dict(f, want=want, loading=loading)


def _interfered(f, kinds, seed, itsc):
    """A copy of two-antenna family f with, on burst b, kinds[b % len(kinds)]'s interferer (None: none) added to both antennas'
    samples: a normal burst of training sequence itsc and random payload through mlse_family.channel with random tap phases per
    antenna, scaled to the stated C/I against that antenna's burst.  amp, TOA and primary stay what the clean bursts gave: they are
    inputs.  want = the diversity model's on the new samples (mlse_irc wants its symbols)."""
    rng = np.random.default_rng(seed)
    sps, B = f["sps"], len(f["off0"])
    o = oraclebind.Oracle(sps)
    ibits = synth.normal_bits(rng, B, itsc)
    x = [f["x0"].copy(), f["x1"].copy()]
    off = [f["off0"], f["off1"]]
    for b in range(B):
        kind = kinds[b % len(kinds)]
        if kind is None:
            continue
        L = int(f["length"][b])
        si = o.modulate(ibits[b].astype(np.int8), 9)
        for a in (0, 1):
            xi = mlse_family.channel(rng, si, sps, mlse_family.PROFILES[kind[0]], None)[:L].astype(np.complex128)
            own = x[a][off[a][b]:off[a][b] + L].astype(np.complex128)
            g = np.sqrt(np.mean(np.abs(own) ** 2) / np.mean(np.abs(xi) ** 2)) * 10.0 ** (-kind[1] / 20.0)
            x[a][off[a][b]:off[a][b] + L] = (own + g * xi).astype(np.complex64)
    want = dm.mlse_div_batch(sps, x[0], f["off0"], x[1], f["off1"], f["length"], f["tsc"], f["amp"], f["toa"], primary=f["primary"], oracle=o)
    return dict(f, x0=x[0], x1=x[1], want=want, interferer=np.array([kinds[b % len(kinds)] is not None for b in range(B)]))


@functools.lru_cache(maxsize=None)
def mixed_batch(sps, tsc, B, seed, loading=im.LOADING):
    """mlse_div_family.mixed_batch (both offset parities, 156- and 157-symbol lengths, TOAs off the grid) with an interferer of
    training sequence (tsc + 3) % 8 on five bursts of six: flat and dispersive, C/I 0 to 10 dB.  want: the IRC model's; want_div:
    the diversity model's on the same samples."""
    f = _interfered(dfam.mixed_batch(sps, tsc, B, seed), INTERFERER_KINDS, seed + 77, (tsc + 3) % 8)
    g = with_model(f, loading)
    g["want_div"] = f["want"]
    return g


@functools.lru_cache(maxsize=None)
def graded_batch(sps, tsc=5, per=24, seed=9100):
    """The family the float64 reference grades: mlse_div_family.graded_batch (3 noise levels x `per` bursts, independent channels
    per antenna) with the interferers above on five bursts of six."""
    f = _interfered(dfam.graded_batch(sps, tsc, per, seed), INTERFERER_KINDS, seed + 78, (tsc + 3) % 8)
    return with_model(f)


@functools.lru_cache(maxsize=None)
def interfered_family(sps, ci_db, snr_db, n, seed, tsc=2, itsc=5, iprofile=None):
    """mlse_div_family.rayleigh_family plus a co-channel handset: n bursts of the "five" profile with independent Rayleigh taps per
    antenna and burst at one MEAN snr, and on each a normal burst of training sequence itsc and random payload through ITS OWN
    independent Rayleigh taps per antenna (profile iprofile, a tuple; None = "five"), scaled to the mean C/I ci_db and added before
    analyzeTrafficBurst.  The draws: the bits, then the interferer's bits; per burst antenna 0's signal, antenna 0's interferer,
    antenna 1's signal, antenna 1's interferer.  dict(o, bits, xs0, xs1, v [n, 2], amp [n, 2], toa [n, 2], sel [n])."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(sps)
    prof = np.asarray(mlse_family.PROFILES["five"], np.complex128)
    iprof = prof if iprofile is None else np.asarray(iprofile, np.complex128)
    pw = np.sqrt(np.sum(np.abs(prof) ** 2)); ipw = np.sqrt(np.sum(np.abs(iprof) ** 2))
    sigma = pw * 10.0 ** (-snr_db / 20.0)
    g = (pw / ipw) * 10.0 ** (-ci_db / 20.0)
    bits = synth.normal_bits(rng, n, tsc); ibits = synth.normal_bits(rng, n, itsc)
    xs0, xs1 = [], []
    v = np.zeros((n, 2), bool); amp = np.zeros((n, 2), np.complex64); toa = np.zeros((n, 2), np.float32)
    for b in range(n):
        s = o.modulate(bits[b].astype(np.int8), 8); si = o.modulate(ibits[b].astype(np.int8), 8)
        xs = []
        for a in range(2):
            x = dfam.rayleigh(rng, s, sps, prof, sigma).astype(np.complex128)
            xi = dfam.rayleigh(rng, si, sps, iprof, 0.0).astype(np.complex128) * g
            xs.append((x + xi).astype(np.complex64))
        xs0.append(xs[0]); xs1.append(xs[1])
        for a, x in enumerate(xs):
            v[b, a], amp[b, a], toa[b, a] = dfam.analyse(o, x, tsc)
    sel = dm.select(v[:, 0], amp[:, 0], v[:, 1], amp[:, 1])
    return dict(o=o, sps=sps, tsc=tsc, bits=bits, xs0=xs0, xs1=xs1, v=v, amp=amp, toa=toa, sel=sel)


def payload_errors(r, loading=im.LOADING):
    """(MRC's, IRC's) payload bit errors on a rayleigh_family / interfered_family dict, an undetected burst counting as half its
    payload bits (tests/test_mlse_div_model.py, test_diversity_pays), and the number of undetected bursts."""
    o, sps, tsc, n = r["o"], r["sps"], r["tsc"], len(r["sel"])
    pay = mlse_family.PAYLOAD
    x0, off0, length = mlse_family.pack(r["xs0"]); x1, off1, _ = mlse_family.pack(r["xs1"])
    sel = r["sel"]
    pick = np.where(sel == 1, 1, 0)
    amp = r["amp"][np.arange(n), pick]; toa = r["toa"][np.arange(n), pick]
    mrc = dm.mlse_div_batch(sps, x0, off0, x1, off1, length, tsc, amp, toa, primary=pick, enable=(sel < 2), oracle=o)
    irc = im.mlse_irc_batch(sps, x0, off0, x1, off1, length, tsc, amp, toa, primary=pick, enable=(sel < 2), loading=loading, y=mrc["y"])

    def errors(soft):
        e = ((soft > 0.5) != r["bits"])[:, pay].sum(axis=1)
        return int(np.where(sel < 2, e, len(pay) // 2).sum())
    return errors(mrc["soft"]), errors(irc["soft"]), int((sel == 2).sum())
