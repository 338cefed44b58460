"""Edge-of-range bursts for the four sequence-equaliser kernels (tests/test_mlse_edge_model.py, tests/test_gpu_mlse_edge.py): the
mixed_batch families of mlse_family, mlse_div_family, mlse_irc_family and mlse_access_family with their samples multiplied by
2^k while amp stays, so that the symbols scale by 2^k -- down to where their squares are subnormal and then zero, up to the 2^30
guard; bursts on the boundaries of k_demod's geometry test; and covariance sets on the boundaries of step 2c.  Test INPUT
generation only; the expected values come from the four float32 models (the one check stated here, assert_scale_identity,
compares a result with itself and needs none).  Computed once, shared; nobody writes to them."""
import functools

import numpy as np

import mlse_access_family
import mlse_access_model
import mlse_div_family
import mlse_div_model
import mlse_family
import mlse_irc_family
import mlse_irc_model as im
import mlse_model

F = np.float32
KERNELS = ("mlse", "div", "irc", "access")
KS = (-75, 0, -74, 28, -73, 29, -72, -50, -70, -66, -60)      # neighbours in this order share a wave
TSC = 2


def kernel_of(f):
    if "x0" in f:
        return "irc" if "loading" in f else "div"
    return "mlse" if "tsc" in f else "access"


def antennas(f):
    """The (samples, offsets) keys of f's antennas."""
    return (("x0", "off0"), ("x1", "off1")) if "x0" in f else (("x", "off"),)


def nbursts(f):
    return len(f["length"])


def model(f, enable=None, cov_in=None, loading=None):
    """The results of f's own model on f."""
    kind = kernel_of(f)
    if kind == "mlse":
        return mlse_model.mlse_batch(f["sps"], f["x"], f["off"], f["length"], f["tsc"], f["amp"], f["toa"], enable=enable)
    if kind == "access":
        return mlse_access_model.access_batch(f["sps"], f["x"], f["off"], f["length"], f["amp"], f["toa"], enable=enable)
    two = (f["sps"], f["x0"], f["off0"], f["x1"], f["off1"], f["length"], f["tsc"], f["amp"], f["toa"])
    if kind == "div":
        return mlse_div_model.mlse_div_batch(*two, primary=f["primary"], enable=enable)
    return im.mlse_irc_batch(*two, primary=f["primary"], enable=enable, loading=f["loading"] if loading is None else loading, cov_in=cov_in)


# the seeds of the base families: the first from 8800 on whose bursts meet every condition of tests/test_mlse_edge_model.py
SEEDS = {("irc", 1): 8803, ("irc", 2): 8804, ("irc", 4): 8802, ("access", 1): 8802, ("access", 2): 8802, ("access", 4): 8802}     # (the others: 8800)


def base_family(kernel, sps, B=6, seed=None):
    """The kernel's own mixed_batch: burst 0 a clean flat one, 2 a noisy five-tap one, 3 a noisy precursor one."""
    seed = SEEDS.get((kernel, sps), 8800) if seed is None else seed
    if kernel == "mlse":
        return mlse_family.mixed_batch(sps, TSC, B, seed)
    if kernel == "div":
        return mlse_div_family.mixed_batch(sps, TSC, B, seed)
    if kernel == "irc":
        return mlse_irc_family.mixed_batch(sps, TSC, B, seed)
    return mlse_access_family.mixed_batch(sps, B, seed)


def rescaled(f, k):
    """f with burst b's samples multiplied by 2^k[b] on every antenna (in float64, then cast to complex64; k a number or [B]) and
    want recomputed by f's model."""
    k = np.broadcast_to(np.asarray(k, np.int64), (nbursts(f),))
    g = {key: v for key, v in f.items() if key not in ("want", "want_div")}
    for xk, ok in antennas(f):
        x = f[xk].astype(np.complex128)
        for b in range(nbursts(f)):
            o, n = int(f[ok][b]), int(f["length"][b])
            if o >= 0:
                x[o:o + n] *= 2.0 ** int(k[b])
        with np.errstate(all="ignore"):
            g[xk] = x.astype(np.complex64)
    g["k"] = k.copy()
    g["want"] = model(g)
    return g


def scaled(f, k):
    """A copy of any of the four mixed_batch dicts with both antennas' samples multiplied by 2^k and want recomputed."""
    return rescaled(f, int(k))


def picked(f, idx, gap_seed=0):
    """Bursts idx (repeats allowed) of f packed anew, gaps of 1 or 2 samples that differ between the antennas; no want."""
    idx = np.asarray(idx)
    n = len(idx)
    g = {key: v for key, v in f.items() if key not in ("want", "want_div", "bits", "ra", "bsic", "interferer", "k")}
    for a, (xk, ok) in enumerate(antennas(f)):
        xs = [f[xk][f[ok][b]:f[ok][b] + f["length"][b]] for b in idx]
        gaps = [1 if (i + a + gap_seed) % 3 == 0 else 2 for i in range(n)] if a == 0 else [2 if (i + gap_seed) % 4 == 1 else 1 for i in range(n)]
        g[xk], g[ok], g["length"] = mlse_family.pack(xs, gaps=gaps)
    for key in ("amp", "toa", "primary"):
        if key in f:
            g[key] = f[key][idx].copy()
    g["base"] = idx.copy()
    return g


BASES = (0, 2, 3)                                              # of base_family: clean flat, noisy five-tap, noisy precursor


def ladder_order():
    """(base, k) of the ladder's 35 bursts.  Burst b < 33 is base b % 3 at KS[b % 11] (3 and 11 are coprime: every pair once), so
    that the bursts 2i, 2i + 1 of a two-burst wave are neighbours in KS -- 2^-75 (falls back) beside 1, 2^-74 beside 2^28, 2^-73
    beside 2^29 -- and the four of a k_mlse_access wave four in a row of it.  Two more (2^-75 and 2^29, the only scales that b % 4
    == 1 and 2 had not seen) make the batch odd and its last wave partial."""
    return [(b % 3, KS[b % 11]) for b in range(33)] + [(0, -75), (1, 29)]


@functools.lru_cache(maxsize=None)
def ladder(kernel, sps, ks=None):
    """One batch of scaled copies of three base bursts, interleaved (ladder_order); ks: only the copies at these scales.  f["base"]
    and f["k"] name each burst."""
    order = [(i, k) for i, k in ladder_order() if ks is None or k in ks]
    base = base_family(kernel, sps)
    g = picked(base, [BASES[i] for i, _ in order])
    g = rescaled(g, [k for _, k in order])
    g["base"] = np.array([i for i, _ in order])
    return g


TRELLIS = {k: np.r_[0:61, 87:148] for k in ("mlse", "div", "irc")}      # the positions the trellis decides (payload, flags, tail)
TRELLIS["access"] = np.arange(49, 88)
PAYLOAD = {k: mlse_family.PAYLOAD for k in ("mlse", "div", "irc")}
PAYLOAD["access"] = mlse_access_family.PAYLOAD


def copies(f, k):
    """The ladder's bursts at scale k, one per base burst, in base order (of two copies of a base the first)."""
    return np.array([np.flatnonzero((f["k"] == k) & (f["base"] == i))[0] for i in range(len(BASES))])


def assert_scale_identity(kernel, out, f, k):
    """The one check that needs no model, on the model's results or a kernel's: rows k of `out` against its rows 0 -- the trellis's soft
    bits, the hard bits there and the window word equal byte for byte, the taps times 2^k exactly, IRC's set unchanged.  (The
    midamble's soft bits are the demodulator's (re + 1) / 2, which does not scale.)"""
    a, z = copies(f, k), copies(f, 0)
    tr = TRELLIS[kernel]
    what = "%s sps %d, 2^%d against 1: " % (kernel, f["sps"], k)
    assert np.all(out["win"][z] <= 0), what + "a base burst is not equalised"
    assert out["soft"][a][:, tr].tobytes() == out["soft"][z][:, tr].tobytes(), what + "soft bits"
    assert out["hard"][a][:, tr].tobytes() == out["hard"][z][:, tr].tobytes(), what + "hard bits"
    assert out["win"][a].tobytes() == out["win"][z].tobytes(), what + "window word"
    taps = np.ldexp(np.ascontiguousarray(out["chan"][z]).view(F), k)
    assert np.ascontiguousarray(out["chan"][a]).view(F).tobytes() == taps.tobytes(), what + "taps"
    if "cov" in out:
        assert out["cov"][a].tobytes() == out["cov"][z].tobytes(), what + "set"


def window_energies(f, want=None):
    """E_w of the five windows in scan order (w = 0, -1, .., -4), [B, 5] float32, as f's model forms them from want["y"]."""
    want = f["want"] if want is None else want
    kind = kernel_of(f)
    y = want["y"]
    with np.errstate(all="ignore"):
        if kind == "mlse":
            c = mlse_model.estimate(y, mlse_model.tsc_symbols(f["tsc"]))[0]
            p = c.real.astype(F) * c.real.astype(F) + c.imag.astype(F) * c.imag.astype(F)
        elif kind == "access":
            c = mlse_access_model.estimate(y)[0]
            p = c.real.astype(F) * c.real.astype(F) + c.imag.astype(F) * c.imag.astype(F)
        else:
            c = mlse_div_model.estimate(y, mlse_model.tsc_symbols(f["tsc"]))[0]
            cr, ci = c.real.astype(F), c.imag.astype(F)
            p = (cr[:, 0] * cr[:, 0] + ci[:, 0] * ci[:, 0]) + (cr[:, 1] * cr[:, 1] + ci[:, 1] * ci[:, 1])
        return np.stack([(((p[:, k] + p[:, k + 1]) + p[:, k + 2]) + p[:, k + 3]) + p[:, k + 4] for k in (4, 3, 2, 1, 0)], axis=1).astype(F)


# ---- bursts on the boundaries of k_demod's test ----

UP, DOWN = F(np.nextafter(F(4096.0), F(np.inf))), F(np.nextafter(F(-4096.0), F(-np.inf)))
EQ, FB, SK = 0, 1, 2                                          # equalised, fell back, skipped


def geometry_cases(sps):
    """(name, symbols or None, samples beyond whole symbols, TOA or None, offset -1, state expected)."""
    plain = ("plain", None, 0, None, False, EQ)
    s91, s92, s147 = ("91 symbols", 91, 0, None, False, SK), ("92 symbols", 92, 0, None, False, FB), ("147 symbols", 147, 0, None, False, FB)
    s148, s157, s158 = ("148 symbols", 148, 0, None, False, EQ), ("157 symbols", 157, 0, None, False, EQ), ("158 symbols", 158, 0, None, False, SK)
    tp, tm = ("TOA 4096", None, 0, F(4096.0), False, FB), ("TOA -4096", None, 0, F(-4096.0), False, FB)
    tpp, tmm = ("TOA past 4096", None, 0, UP, False, SK), ("TOA past -4096", None, 0, DOWN, False, SK)
    tnan, neg = ("TOA NaN", None, 0, F(np.nan), False, SK), ("offset -1", None, 0, None, True, SK)
    cases = [plain, s91, s92, plain, s147, s158, s148, s157, tp, tm, tpp, tmm, tnan, plain, neg, s92, plain, s147, neg, plain, s158, tp,
             plain, tnan]                                      # (read in pairs: every ordered pair of states is there)
    if sps > 1:
        cases += [("150 symbols and a sample", 150, 1, None, False, SK), plain, ("149 symbols less a sample", 148, sps - 1, None, False, SK)]
    else:
        cases += [s91, plain, s148]
    return cases


GUARD = 16                                                     # samples in front of the geometry batch's arrays


@functools.lru_cache(maxsize=None)
def geometry(kernel, sps):
    """27 bursts on the boundaries of k_demod's test between ordinary ones (geometry_cases): lengths of 91, 92, 147, 148, 157 and
    158 symbols, at sps 2 and 4 lengths that are no multiple of sps, TOA = +-4096 exactly (the delayed burst is all zeros: E == 0) and
    one float beyond, a NaN TOA, offset -1.  For the two-antenna kernels the negative offset is the non-primary antenna's alone, and so
    is the short length as far as that can be: the antennas share d_length, but the primary antenna's array keeps the whole burst
    behind it while the other's is cut there.  Every ordered pair of (equalised, fell back, skipped) is a wave's (bursts 2i, 2i + 1).
    The first GUARD samples of each array are padding: the callers hand the kernels a view that starts behind them, so that a read
    at offset -1 stays inside the allocation.  f["name"] and f["state"] describe each burst."""
    cases = geometry_cases(sps)
    base = base_family(kernel, sps)
    n = len(cases)
    idx = np.array([BASES[i % 3] for i in range(n)])
    two = kernel in ("div", "irc")
    g = {key: v for key, v in base.items() if key not in ("want", "want_div", "bits", "ra", "bsic", "interferer")}
    amp = base["amp"][idx].copy(); toa = base["toa"][idx].copy()
    primary = base["primary"][idx].copy() if two else np.zeros(n, np.uint8)
    if two:
        g["primary"] = primary
    length = np.zeros(n, np.int32)
    for a, (xk, ok) in enumerate(antennas(base)):
        xs = []
        for i, (name, nsym, extra, t, neg, state) in enumerate(cases):
            b = idx[i]
            x = base[xk][base[ok][b]:base[ok][b] + base["length"][b]]
            length[i] = len(x) if nsym is None else nsym * sps + extra
            if nsym is not None:
                keep = max(length[i], len(x)) if two and a == primary[i] else length[i]      # (the primary antenna's array keeps the whole burst)
                x = np.r_[x, np.zeros(2 * sps, np.complex64)][:keep]
            xs.append(np.ascontiguousarray(x))
            if t is not None:
                toa[i] = t
        x, off, _ = mlse_family.pack(xs, gaps=[GUARD + 1 + a] + [1 + (i + a) % 2 for i in range(1, n)])
        for i, c in enumerate(cases):
            if c[4] and (not two or a != primary[i]):
                off[i] = -1
        g[xk], g[ok] = x, off
    g["length"] = length
    g["amp"], g["toa"] = amp, toa
    g["name"] = [c[0] for c in cases]
    g["state"] = np.array([c[5] for c in cases])
    g["want"] = model(g)
    return g


# ---- covariance sets on the boundaries of step 2c ----

L10 = F(np.nextafter(F(1024.0), F(0.0)))
U1 = F(np.nextafter(F(1.0), F(0.0)))


def irc_sets():
    """[(d_cov_in row, accepted)]: rows on the boundaries that the invalid-set test steps over.  accepted: the set is used and
    reported as given; otherwise the identity set is."""
    return [
        ((L10, 1, 0, 0), True),                                # the largest A below 2^10
        ((1, L10, 0, 0), True),                                # the largest Bv
        ((L10, L10, 1023, 0), True),                           # both, beside a large xr: det = L10^2 - 1023^2 > 0
        ((L10, L10, L10, 0), False),                           # the largest xr passes the magnitude test, but no diagonal below 2^10 outweighs it: det = 0
        ((L10, L10, 0, -L10), False),                          # ... nor the largest |xi|
        ((L10, L10, 0, 1023), True),                           # xi one step inside that
        ((-0.0, 1, 0, 0), False),                              # -0 >= 0 holds, det = -0 is not > 0
        ((1, -0.0, 0, 0), False),
        ((1, 1, U1, 0), True),                                 # det = 1 - fl(U1^2) = 2^-23: antenna 0 all but nulled
        ((1, 1, 0, -U1), True),
        ((F(1 + 2.0 ** -23), F(1 - 2.0 ** -24), 1, 0), False),  # A Bv = 1 + 2^-24 - 2^-47 rounds to 1 = |x|^2: det = 0 though the real one is positive
        ((F(2.0 ** -126), 1, 0, 0), True),                     # the smallest normal diagonal: det = 2^-126
        ((1, F(2.0 ** -126), 0, 0), True),
        ((F(2.0 ** -140), 1, 0, 0), True),                     # a subnormal one: det = 2^-140 > 0 only if nothing flushes it
        ((1, F(2.0 ** -149), 0, 0), True),                     # the smallest subnormal
        ((F(2.0 ** -126), F(2.0 ** -126), 0, 0), False),       # the product underflows to 0
    ]


@functools.lru_cache(maxsize=None)
def irc_set_batch(sps):
    """One burst per irc_sets() row (the base family's, in turn): f["cov_in"] [B, 4], f["accepted"] [B], want the model's with them."""
    rows = irc_sets()
    base = base_family("irc", sps)
    f = picked(base, np.arange(len(rows)) % nbursts(base))
    f["cov_in"] = np.array([r for r, _ in rows], F)
    f["accepted"] = np.array([a for _, a in rows], bool)
    f["want"] = model(f, cov_in=f["cov_in"])
    return f


def estimated_set_cases(sps, B=9):
    """[(name, two-antenna family without want, loading, identity expected)] for the estimated set: antenna 1 a copy of antenna 0
    (S00 == S11 == Xr, Xi == 0: A == Bv == xr == 0.5 exactly at loading 0, det == 0, the identity set), antenna 1 twice antenna 0
    (A = 0.2, Bv = 0.8, xr = 0.4 in exact arithmetic: det is rounding error, the model decides) and the copy at loading 2^-20, where
    det is about 2^-20 and the set is used."""
    one = base_family("mlse", sps, 9, 8850)
    assert B <= nbursts(one)
    sel = np.arange(B)
    f = dict(sps=sps, tsc=one["tsc"], x0=one["x"], off0=one["off"][sel], x1=one["x"], off1=one["off"][sel], length=one["length"][sel],
             amp=one["amp"][sel], toa=one["toa"][sel], primary=np.zeros(B, np.uint8))
    twice = dict(f, x1=(2.0 * one["x"].astype(np.complex128)).astype(np.complex64))
    return [("copy, loading 0", f, F(0.0), True), ("twice, loading 0", twice, F(0.0), None), ("copy, loading 2^-20", f, F(2.0 ** -20), False)]
