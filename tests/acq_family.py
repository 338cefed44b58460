"""An adversarial family of streams for mobile-side acquisition (include/trxsig_l1acq.h; csrc/trxsig_l1acq.hip and .cpp), and
the exact model that says -- on the CPU alone -- what the library must answer for them.  CPU only: no native library is loaded
here except the oracle's primitives the stream builder of tests/l1_acq_model.py uses.

Stage 1 has no reference to be bit-identical to, and the order of the additions inside a scan is the implementation's, so in
general it is graded through a tolerance.  ON A LATTICE STREAM IT CAN BE GRADED WITH ==: where every d[n] and e[n] is a multiple
of one power of two (the granule) and the sum of the magnitudes of any L consecutive ones stays below 2^24 granules, every
float32 partial sum of at most L of them is exact IN ANY ORDER, so C[k] and E[k] are determined; m[k] is three rounded float32
operations on them in the order the header writes, so it is determined too, and with it the smallest k of the largest m.
lattice_model() forms those sums in integers, asserts the lattice condition and returns the answer.

Lattice members (lattice_members(sps); every stream has N = 70 * 1136 + 333 samples: 71 tiles of the first launch at sps 1 and
2, 70 at sps 4 -- more than the 64 lanes of the second launch either way; the streams are j^walk[n // sps], amplitudes 1,
2^-6 and 0):
  plateau       the tone j^(n // sps) throughout: every window scores exactly 1.0 -- the answer is k = 0
  late_plateau  P zeros, then the tone, P on both sides of the thread stride (256), the window (L), the tile (1136) and the 64th
                tile: k = P, the partly filled windows before it score less
  twin_runs     a unit-modulus random walk (steps from {+1, +1, +1, 0, 2, 3}, no more than 40 steps of +1 in a row) with
                identical tone runs of L + sps samples planted in it, each scoring exactly 1.0: two in one tile under different
                waves; two in one tile under the same thread; in tiles t and t + 64 (one lane of the pick); in tiles 63 and 64
                (the later tile in an earlier lane); across a tile boundary; across a segment boundary inside a tile.  The
                earliest run must win.
  quiet_twin    the same with the runs at amplitude 2^-6 beside the unit fill.  (2^-6 holds the lattice condition at every sps:
                the granule of e is 2^-13 and the largest window sum, L = 568 at sps 4, is 4.7e6 granules.)  A differenced running
                sum is not exact here -- its 80,000-term prefix leaves the lattice -- so this member is graded against the exact
                sums and the segment emulation only.
  border        the constant stream, (-1)^(n // sps) and (-j)^(n // sps): Re C is exactly 0, 0 and -L in every window, so every
                window scores 0: k = 0, C = (0, -L), (0, +L), (-L, 0), arg = -pi / 2, +pi / 2, pi
  threshold     the random walk with one tone run in which 5 of the 142 steps are 3 instead of 1: C = L - 10 sps exactly, E = L,
                0.5 < m < 1 known exactly; with plateau (m = 1.0) the two streams whose m a threshold can be set equal to

Not lattice, graded by the header's tolerances:
  angle_sweep    63 tones A exp(j (pi / 2 + theta) n / sps): every octant of atan2, both half planes, 0.01 rad either side of
                 the Re C = 0 border
  far_offset     a frame of fill and two frames (FCCH, then SCH) at 20 dB, rotated by +-0.2 and +-0.24 cycle / symbol
  dynamic_range  one quiet frequency burst with every other slot 60 dB and 90 dB up

WHAT THE CPU MODEL REACHES ON ITS OWN k (am.search_model; recorded here, asserted in tests/test_acq_family.py, demanded of the
library in tests/test_gpu_acq_family.py):
  far_offset     state 15 in all twelve cases (sps 1, 2, 4; f = +0.2, -0.2, +0.24, -0.24)       -> FAR_OFFSET_STATE
  sps-2 truth    16 of the 16 cases of am.truth_cases(2) reach state 15                          -> TRUTH2_STATE15

Helper module, no tests here (tests/test_acq_family.py proves the family is what it claims, tests/test_gpu_acq_family.py grades
the kernels)."""
import functools

import numpy as np

import fectxbind
import l1_acq_model as am
import oraclebind

F32 = np.float32
SPS = (1, 2, 4)
W = 1136                                                       # window starts per tile of the first launch, at any sps
N_LATTICE = 70 * W + 333
UNIT = np.array([1, 1j, -1, -1j], np.complex64)
QUIET = 2.0 ** -6
FAR_F = (0.2, -0.2, 0.24, -0.24)
FAR_OFFSET_STATE = {(sps, f): 15 for sps in SPS for f in FAR_F}
TRUTH2_STATE15 = 16


@functools.lru_cache(maxsize=None)
def oracle(sps):
    return oraclebind.Oracle(sps)


@functools.lru_cache(maxsize=None)
def fec_tx():
    return fectxbind.FecTxOracle()


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- the exact model -------------------------------------------------------------------------------------------------------
def metric32(C, E):
    """m as the header writes it, in float32: |C|^2 and E^2 first, one division; 0 unless Re C > 0, E > 0 and all finite"""
    cr, ci, e = np.asarray(C).real.astype(F32), np.asarray(C).imag.astype(F32), np.asarray(E).astype(F32)
    with np.errstate(all="ignore"):
        q = (cr * cr + ci * ci) / (e * e)
        ok = (cr > 0) & (e > 0) & np.isfinite(cr) & np.isfinite(ci) & np.isfinite(e) & np.isfinite(q)
    return np.where(ok, q, F32(0)).astype(F32)


def _granule(v):
    """the largest power of two of which every entry of v is a multiple (1 where v is all zero)"""
    nz = v[v != 0]
    if len(nz) == 0:
        return 1.0
    for q in range(-8, 64):
        g = 2.0 ** -q
        if (nz / g == np.rint(nz / g)).all():
            return g
    raise AssertionError("not a lattice stream: no granule down to 2^-63")


def lattice_model(x, sps):
    """The exact stage-1 answer for a lattice stream: dict(k, m, C, E) at the first argmax, and C_all, E_all, m_all over every
    window start.  Asserts the lattice condition: every float32 product and sum that forms d and e is exact, and for each of
    Re d, Im d and e the sum of the magnitudes over any window is below 2^24 granules -- so every partial sum of at most L of
    them, in any order, is exactly representable in float32."""
    x = np.asarray(x, np.complex64)
    L, N = am.fcch_len(sps), len(x)
    assert N >= L + sps, "the stream has no window"
    xr, xi = x.real.astype(np.float64), x.imag.astype(np.float64)
    ar, ai, br, bi = xr[sps:], xi[sps:], xr[:-sps], xi[:-sps]

    def exact(v):                                              # float64 holds it exactly; does float32?
        assert (v == v.astype(F32)).all(), "not a lattice stream: a term is not exact in float32"
        return v
    dr = exact(exact(ai * br) - exact(ar * bi))
    di = -exact(exact(ar * br) + exact(ai * bi))
    e = exact(0.5 * exact(exact(exact(br * br) + exact(bi * bi)) + exact(exact(ar * ar) + exact(ai * ai))))
    sums, granules = [], []
    for v in (dr, di, e):
        g = _granule(v)
        iv = np.rint(v / g).astype(np.int64)
        assert (iv * g == v).all()
        cs = np.concatenate([[0], np.cumsum(iv)])
        ca = np.concatenate([[0], np.cumsum(np.abs(iv))])
        assert (ca[L:] - ca[:-L]).max() < 2 ** 24, "not a lattice stream: a partial sum may leave 24 bits"
        sums.append((cs[L:] - cs[:-L]) * g)                    # exact: an integer below 2^24 times a power of two
        granules.append(g)
    C, E = (sums[0] + 1j * sums[1]).astype(np.complex64), sums[2].astype(F32)
    assert (C.real == sums[0]).all() and (C.imag == sums[1]).all() and (E == sums[2]).all()
    m = metric32(C, E)
    k = int(np.argmax(m))                                      # the first of the largest
    return dict(k=k, m=m[k], C=C[k], E=E[k], C_all=C, E_all=E, m_all=m, granules=tuple(granules))


def plateaus(m, value=1.0):
    """[(first k, last k)] of the maximal runs of window starts whose metric equals value"""
    hit = np.flatnonzero(m == F32(value))
    if len(hit) == 0:
        return []
    cut = np.flatnonzero(np.diff(hit) > 1)
    return list(zip(hit[np.concatenate([[0], cut + 1])].tolist(), hit[np.concatenate([cut, [len(hit) - 1]])].tolist()))


# ---- lattice members -------------------------------------------------------------------------------------------------------
def tone(n, sps, step=1):
    """j^(step * (i // sps)) for i < n, exactly"""
    return UNIT[(step * (np.arange(n) // sps)) % 4]


@functools.lru_cache(maxsize=None)
def _walk():
    """one symbol walk for every sps: steps from {+1, +1, +1, 0, 2, 3}, no more than 40 steps of +1 in a row"""
    rng = np.random.default_rng(4601)
    steps = rng.choice(np.array([1, 1, 1, 0, 2, 3]), N_LATTICE + 1)
    run = 0
    for i in range(len(steps)):
        run = run + 1 if steps[i] == 1 else 0
        if run > 40:
            steps[i], run = (0, 2, 3)[i % 3], 0
    return _frozen(np.cumsum(steps) % 4)


def fill(sps):
    return UNIT[_walk()[np.arange(N_LATTICE) // sps]].copy()


def late_positions(sps):
    L = am.fcch_len(sps)
    return (1, 255, 256, 257, L - 1, L, L + 1, W - 1, W, W + 1, 64 * W - 1, 64 * W, 64 * W + 1)


# (name, [(tile, index in the tile) of each run's first window start]); L stands for the segment length
TWIN = (("one tile, waves 0 and 2", ((5, 10), (5, 650))),
        ("one tile, one thread", ((7, 10), (7, 778))),
        ("tiles 3 and 67", ((3, 300), (67, 300))),
        ("tiles 63 and 64", ((63, 500), (64, 20))),
        ("across a tile boundary", ((8, W - 50), (20, 400))),
        ("across a segment boundary", ((30, "L-50"), (40, 100), (41, 900))))


def twin_positions(sps, where):
    L = am.fcch_len(sps)
    return [t * W + (L - 50 if i == "L-50" else i) for t, i in where]


def _twin(sps, where, amp):
    L = am.fcch_len(sps)
    R = L + sps
    x = fill(sps)
    at = twin_positions(sps, where)
    assert all(b - a >= R + 2 * sps for a, b in zip(at, at[1:])) and at[0] >= sps and at[-1] + R + sps <= N_LATTICE
    for p in at:
        run = tone(R, sps)
        x[p:p + R] = (run * F32(amp)).astype(np.complex64)
        x[p - sps:p] = 1j * run[0]                             # a step of 3 on either side: d = -1 there, so the run's own
        x[p + R:p + R + sps] = -1j * run[-1]                   # window is the only one of its neighbourhood that scores 1.0
    lm = lattice_model(x, sps)
    pl = plateaus(lm["m_all"])
    # each run's own window scores exactly 1.0, nothing else does, and the earliest run wins
    assert len(at) >= 2 and pl == [(p, p) for p in at], (sps, where, pl, at)
    assert lm["m"] == 1.0 and lm["m_all"].max() == 1.0 and lm["k"] == at[0]
    return x, dict(runs=at, plateaus=pl)


def threshold_stream(sps):
    """the random walk, and one tone run of L + sps samples in it whose steps 20, 45, 70, 95 and 120 are 3 instead of 1 (with a
    step of 3 on either side like the twin runs).  Silence round the run will not do: the windows that hold only the run's last
    21 symbols score 0.95, more than the run's own 0.86."""
    L = am.fcch_len(sps)
    steps = np.ones(142, np.int64)
    steps[[20, 45, 70, 95, 120]] = 3
    walk = np.concatenate([[0], np.cumsum(steps)]) % 4
    x = fill(sps)
    p = 17 * W + 391
    run = UNIT[walk[np.arange(L + sps) // sps]]
    x[p:p + L + sps] = run
    x[p - sps:p] = 1j * run[0]
    x[p + L + sps:p + L + 2 * sps] = -1j * run[-1]
    return x, p


@functools.lru_cache(maxsize=None)
def lattice_members(sps):
    """[dict(name, x, model, unit, expect, ...)]: model is lattice_model(x, sps); unit: amplitudes 0 and 1 only (a differenced
    running sum is exact too); expect: what the family's description promises (k, m, C, E, arg), checked against the model in
    tests/test_acq_family.py"""
    L, N = am.fcch_len(sps), N_LATTICE
    out = []

    def add(name, x, unit=True, expect=None, **more):
        x = _frozen(np.ascontiguousarray(x, np.complex64))
        assert len(x) == N
        out.append(dict(name=name, x=x, model=lattice_model(x, sps), unit=unit, expect=expect or {}, **more))
    add("plateau", tone(N, sps), expect=dict(k=0, m=1.0, C=L + 0j, E=L))
    for P in late_positions(sps):
        add("late_plateau %d" % P, np.concatenate([np.zeros(P, np.complex64), tone(N - P, sps)]),
            expect=dict(k=P, m=1.0, C=L + 0j, E=L))
    for name, where in TWIN:
        x, info = _twin(sps, where, 1.0)
        add("twin_runs " + name, x, tiles=[t for t, _ in where], **info)
    for name, where in TWIN:
        x, info = _twin(sps, where, QUIET)
        add("quiet_twin " + name, x, unit=False, tiles=[t for t, _ in where], **info)
    for name, step, C, arg in (("constant", 0, -1j * L, -np.pi / 2), ("alternating", 2, 1j * L, np.pi / 2), ("reversed tone", 3, -L + 0j, np.pi)):
        add("border " + name, tone(N, sps, step), expect=dict(k=0, m=0.0, C=C, E=L, arg=arg))
    x, p = threshold_stream(sps)
    add("threshold", x, expect=dict(k=p, C=L - 10 * sps + 0j, E=L))
    m = out[-1]["model"]["m"]
    assert 0.5 < m < 1.0 and m == F32(F32((L - 10 * sps) ** 2) / F32(L * L))
    return out


def exact_m_members(sps):
    """the two streams whose m is known exactly and lies above 0.5: a threshold can be set equal to it"""
    return [mb for mb in lattice_members(sps) if mb["name"] in ("plateau", "threshold")]


# ---- every angle -----------------------------------------------------------------------------------------------------------
def sweep_angles():
    e = np.pi / 8
    named = [s * v for v in (e, 2 * e, 3 * e, 5 * e, 6 * e, 7 * e) for s in (1, -1)]
    near = [s * (np.pi / 2 + d) for d in (-0.01, 0.01) for s in (1, -1)]
    th = np.concatenate([np.linspace(-np.pi + 0.01, np.pi - 0.01, 47), named, near])
    assert len(th) == 63
    return _frozen(th)


def sweep_guard(sps):
    """|Re C64| / E64 must exceed this in every window: then the float64 model and the float32 kernel, whose C is within
    2 (L + 8) 2^-24 E of it (the header's bound), agree on the half plane"""
    return 2 * (am.fcch_len(sps) + 8) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def angle_sweep(sps):
    """(theta[63], [x]): streams of L + 3 sps samples A exp(j (pi / 2 + theta) n / sps), A in [0.3, 3]: C = L A^2 e^(j theta)"""
    L = am.fcch_len(sps)
    th = sweep_angles()
    A = np.random.default_rng(4700 + sps).uniform(0.3, 3.0, len(th))
    n = np.arange(L + 3 * sps)
    xs = [_frozen((a * np.exp(1j * (np.pi / 2 + t) * n / sps)).astype(np.complex64)) for a, t in zip(A, th)]
    for t, x in zip(th, xs):                                   # all 63, nothing dropped
        C, E, _ = am.fcch_metric64(x, sps)
        assert len(C) == 2 * sps + 1 and (np.abs(C.real) > sweep_guard(sps) * E).all(), (sps, t)
    return th, xs


# ---- far offsets and dynamic range -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def far_offset(sps):
    """[(f, x)]: a frame of fill, two frames that start with FCCH and SCH, and two slots, cut in, delayed, rotated by f cycle / symbol, 20 dB"""
    out = []
    for i, f in enumerate(FAR_F):
        rng = np.random.default_rng(4800 + 10 * sps + i)
        clean, _ = am.build_stream(oracle(sps), fec_tx(), rng, 9, 3, 21 + i)      # FCCH in frame 1, SCH in frame 2
        out.append((f, am.impair(clean, rng, sps, 5 + 37 * i * sps, 1 + i, f, 0.9 - 0.3j, 20.0)))
    n = min(len(x) for _, x in out)                            # one length: one search takes them all
    return [(f, _frozen(x[:n].copy())) for f, x in out]


@functools.lru_cache(maxsize=None)
def dynamic_range(sps):
    """[(dB, x)]: one frequency burst (and the SCH behind it) at amplitude 1, every other slot 60 dB and 90 dB up -- 90 dB is
    the range of an int16 radio; no noise.  Asserts that the float32 segment scheme holds the tolerance where it matters."""
    out = []
    for i, db in enumerate((60, 90)):
        rng = np.random.default_rng(4900 + 10 * sps + i)
        clean, _ = am.build_stream(oracle(sps), fec_tx(), rng, 9, 3, 9, keep={1, 2}, loud=10.0 ** (db / 20.0))
        x = _frozen(am.impair(clean, rng, sps, 11, 0, (-0.07, 0.05)[i], 1.0, None))
        m64 = am.fcch_metric64(x, sps)[2]
        k = int(np.argmax(m64))
        seg = am.fcch_metric32_segments(x, sps)
        assert m64[k] > 0.9 and abs(float(seg[k]) - m64[k]) <= am.fcch_tol(sps), (sps, db, m64[k], seg[k])
        out.append((db, x))
    return out
