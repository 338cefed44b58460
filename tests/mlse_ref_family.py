"""The seeded burst family that grades the sequence equaliser against its float64 reference (tests/mlse_ref.py): built as
mlse_family.mixed_batch builds its bursts -- the oracle's modulator, mlse_family.channel, amplitude and TOA from the oracle's
analyzeTrafficBurst, the float32 model's results attached -- in batches of one rate and one training sequence, 319 bursts in all.
Test INPUT generation only.  Every burst carries a name, its noise level (the group the exclusion cap is counted in) and its
group; the members:

  windows   profile "five" at 15 dB, every training sequence, the TOA moved by -4..4 whole symbols: every window w = -4..0
  lone      the flat channel without noise, the TOA moved by -4..4 symbols: the main tap lands on each of h[0]..h[4].  The members
            moved by -4 and +4 put it on h[0] and h[4]: symbol 3 (144) then reaches the left (right) half only through the taps
            behind (ahead of) the main one -- here the modulating pulse's own neighbours, a fifth of it -- and is named in EDGE
  channels  two equal taps four symbols apart, five taps of equal magnitude, an ascending (maximum-phase) profile; random tap
            phases; without noise and at 15 dB
  noise     "five" and "precursor" without noise and at 15, 6 and 0 dB (many near-equal competing paths at the low ones)
  scale     the caller's amplitude times 2^k, k = -20, -10, 0, 10, 20: exact, the symbols scale by 2^-k and E by 2^-2k
  rates     windows (two training sequences), lone and channels again at sps 2 and 4; everything else is at sps 1
Every third burst of a batch has 157 symbols and the gaps alternate between 1 and 2 samples (odd offsets: the non-wide staging
path at sps 2 and 4)."""
import functools

import numpy as np

import mlse_family
import mlse_model
import oraclebind
import synth

PROFILES = dict(mlse_family.PROFILES)
PROFILES.update({
    "two": [0.7071, 0.0, 0.0, 0.0, 0.7071],
    "equal": [0.4472, 0.4472, 0.4472, 0.4472, 0.4472],
    "ascending": [0.1, 0.2, 0.4, 0.7, 1.0],
})
SCALES = (-20, -10, 0, 10, 20)
SHIFTS = tuple(range(-4, 5))
LONE_AT_H0, LONE_AT_H4 = 4, -4                                # the TOA shift (symbols) that lands the lone tap on h[0] / h[4]
EDGE = {LONE_AT_H0: 3, LONE_AT_H4: 144}                       # ... and the symbol one half then barely observes


def _plan(sps):
    """[(tsc, [(name, group, profile, snr, shift, k), ...]), ...]: the batches of one rate."""
    by_tsc = {}

    def add(tsc, name, group, profile, snr, shift=0, k=0):
        by_tsc.setdefault(tsc, []).append((name, group, profile, snr, shift, k))
    for tsc in (range(8) if sps == 1 else (1, 6)):
        for s in SHIFTS:
            add(tsc, "window tsc %d shift %+d" % (tsc, s), "windows", "five", 15.0, s)
    for s in SHIFTS:
        add(2, "lone shift %+d" % s, "lone", "flat", None, s)
    for prof in ("two", "equal", "ascending"):
        for snr in (None, 15.0):
            for i in range(4 if sps == 1 else 1):
                add(2, "%s %s #%d" % (prof, snr, i), "channels", prof, snr)
    if sps == 1:
        for prof in ("five", "precursor"):
            for snr in (None, 15.0, 6.0, 0.0):
                for i in range(16):
                    add(5, "%s %s #%d" % (prof, snr, i), "noise", prof, snr)
            for k in SCALES:
                for i in range(2):
                    add(3, "%s x 2^%d #%d" % (prof, k, i), "scale", prof, 15.0, 0, k)
    return sorted(by_tsc.items())


@functools.lru_cache(maxsize=None)
def batches(sps):
    """The family's batches at one rate: a list of dicts as mlse_family.mixed_batch returns them, plus name, group, snr (NaN = no
    noise), shift and k per burst.  Computed once, shared; nobody writes to them."""
    o = oraclebind.Oracle(sps)
    out = []
    for tsc, members in _plan(sps):
        rng = np.random.default_rng(7300 + 10 * sps + tsc)
        B = len(members)
        bits = synth.normal_bits(rng, B, tsc)
        xs, amp, toa = [], [], []
        shared = {}                                            # a group whose members differ in the TOA alone shares its samples
        for b, (name, group, prof, snr, shift, k) in enumerate(members):
            if group in ("windows", "lone") and group in shared:
                bits[b], x, a, t = shared[group]
            else:
                x = mlse_family.channel(rng, o.modulate(bits[b].astype(np.int8), 9 if (b + tsc) % 3 == 0 else 8), sps, PROFILES[prof], snr)
                r = o.analyze_traffic(x, tsc)
                a, t = (r["amp"], r["toa"]) if r["ok"] and r["amp"] != 0 else (np.complex64(800 - 300j), np.float32(0.0))
                shared[group] = (bits[b].copy(), x, a, t)
            xs.append(x); amp.append(np.complex64(a * np.float32(2.0 ** k))); toa.append(np.float32(t + np.float32(shift * sps)))
        x, off, length = mlse_family.pack(xs, gaps=[1 if b % 2 == 0 else 2 for b in range(B)])
        amp = np.array(amp, np.complex64); toa = np.array(toa, np.float32)
        want = mlse_model.mlse_batch(sps, x, off, length, tsc, amp, toa, oracle=o)
        out.append(dict(sps=sps, tsc=tsc, bits=bits, x=x, off=off, length=length, amp=amp, toa=toa, want=want,
                        name=[m[0] for m in members], group=np.array([m[1] for m in members]),
                        snr=np.array([np.nan if m[3] is None else m[3] for m in members]),
                        shift=np.array([m[4] for m in members]), k=np.array([m[5] for m in members])))
    return out


def family():
    """Every batch, sps 1, 2 and 4."""
    return [f for sps in (1, 2, 4) for f in batches(sps)]


def named_edges(f):
    """[B, 148] bool: the named barely-observed edge symbols of batch f (the lone-tap members moved onto h[0] and h[4])."""
    m = np.zeros((len(f["name"]), 148), bool)
    for b in np.flatnonzero(f["group"] == "lone"):
        if int(f["shift"][b]) in EDGE:
            m[b, EDGE[int(f["shift"][b])]] = True
    return m
