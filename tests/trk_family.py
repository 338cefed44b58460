"""An adversarial family of inputs for the tracking receiver (include/trxsig_l1trk.h; csrc/trxsig_l1trk.hip and .cpp), and the
sharper model of its FCCH records.  CPU only: nothing here loads the library; the oracle's tables come in through the TrkModel
the caller hands over.

THE RECORDS.  The header forms d[n] and e[n] in float32, every product and sum separately rounded, and sums them in float64 in
any order.  fcch_terms32 is that definition literally, fcch_exact sums the terms with math.fsum and states the any-order bound,
and ExactTrk is a TrkModel whose slice carries those records instead of TrkModel.fcch's float64 ones.  On a lattice cell (every
term a multiple of one power of two, the sum of the magnitudes below 2^53 granules) the float64 sum is exact in any order and
the records are compared with ==.

Members (each a dict: x [n_cols][n] complex64, phone, c0, anchors (the arguments of set), n0, fn, F, max_frames, kw (create's
keyword arguments) and what the description promises):
  loop_reuse    204 columns on 68 phones of 3, F = 11 from FN % 51 == 0: 80 workgroups per column over 88 rows, so workgroups
                0 .. 7 form two cells and workgroup 0 forms both FCCH cells (t = 0 and 80).  In every C0 column one of the two
                frequency bursts is a tone with a residual and the other is noise of the same power (even phones: the tone
                first), so a record formed from a stale y[] or red[] is wrong.  Some phones have no C0 column, two are unlocked,
                the anchors stand a frame behind, on and a frame ahead of the call.
  loop_three    the same on 400 columns (133 phones, the last of 4 columns), sps 1: 40 workgroups per column, workgroup 0
                forms t = 0 (FCCH), 40 (not), 80 (FCCH)
  lattice       step 0, phase 0: expjLookup gives exactly (1, 0) and the cell is the stream.  plateau (C = E = L), the three
                borders (Re C = 0, 0, -L), mixed (runs at 2^10 and 2^-10 in one burst: exact in float64, not in float32) and
                threshold (acq_family's run with 5 steps of 3: C = L - 10 sps, E = L), with the pairs of thresholds at which the
                strict > decides
  overflow      a tone at 3e19 (e[n] overflows float32, the samples do not) and at 1e-23 (every term underflows to 0)
  nonfinite     samples with exactly one component NaN (both signs) or +-Inf: in ordinary cells, at a cell's first and last
                sample, inside a frequency burst's measured span; a column whose step is zero and one whose step is not
  capacity      max_frames 52 from FN % 51 == 40 (6 records = the capacity, across the multiframe), max_frames 41 from 0 (5 of
                5), and max_frames 21 from 41 (the first record belongs to frame 10 of the call: j is not f / 10)
  many_phones   200 phones, 3 columns on phones 0, 0 and 199, ten phones unlocked, a seed whose sources put phones 63, 64, 127,
                128 and 199 each in another class
  update_edges  results the test builds with group_result: llrint ties, adj at exact halves, the widest gate, 60 rows at
                -2^24, afc_shift 0 and 8 with a residual of either sign, a phone with no column

Helper module, no tests here (tests/test_trk_family.py proves the family is what it claims, tests/test_gpu_trk_family.py grades
the kernels)."""
import math

import numpy as np

import acq_family as af
import l1_trk_model as ltm

F32 = np.float32
HYPER = ltm.HYPER
M32 = ltm.M32
SPS = (1, 2, 4)
TRK_WG = 16384                                                 # kTrkWg of csrc/trxsig_l1trk.hip: the workgroups of one slice launch
U53 = 2.0 ** -53


def grid_x(n_cols, F):
    """trx_launch_l1trk_slice's rule: workgroups per column"""
    return min(max(TRK_WG // n_cols, 1), 8 * F)


# ---- the records, as the header defines them ----------------------------------------------------------------------------
def fcch_terms32(y, sps):
    """(dr, di, ee): the header's terms over n = 3 sps .. 3 sps + 142 sps - 1 with b = y[n], a = y[n + sps], every operation
    one float32 numpy operation: dr = a.i b.r - a.r b.i, di = -(a.r b.r + a.i b.i), ee = 0.5f ((b.r^2 + b.i^2) + (a.r^2 + a.i^2))"""
    y = np.asarray(y, np.complex64)
    n = 3 * sps + np.arange(142 * sps)
    br, bi = y.real[n].astype(F32), y.imag[n].astype(F32)
    ar, ai = y.real[n + sps].astype(F32), y.imag[n + sps].astype(F32)
    with np.errstate(all="ignore"):
        p1, p2 = ai * br, ar * bi
        dr = p1 - p2
        p3, p4 = ar * br, ai * bi
        di = -(p3 + p4)
        eb, ea = br * br + bi * bi, ar * ar + ai * ai
        ee = F32(0.5) * (eb + ea)
    assert dr.dtype == di.dtype == ee.dtype == F32
    return dr, di, ee


def fcch_exact(y, sps, thresh):
    """The record of a derotated TN 0 cell y: C and E are math.fsum (the correctly rounded exact sum) of fcch_terms32, ok the
    header's rule in double.  abs_c = sum (|dr| + |di|) and abs_e = sum |ee| carry the summation bound n 2^-53 abs, n = 142 sps:
    a float64 sum of n terms in ANY order is within gamma_(n-1) sum |x| of the exact sum, gamma_k = k u / (1 - k u), u = 2^-53,
    and n u dominates gamma_(n-1) because n (n - 1) 2^-53 <= 1.  (For C the bound is on the modulus of the complex error: it
    is at most the sum of the two components' errors.)  The terms come along so that a grader can form exact sum - value
    without a rounding of its own.  Where a term is not finite: finite False, ok False, and C, E hold what any order of
    additions gives (NaN, or the infinity every infinite term agrees on)."""
    dr, di, ee = (v.astype(np.float64) for v in fcch_terms32(y, sps))
    n = 142 * sps
    out = dict(terms=(dr, di, ee), n=n)
    if not (np.isfinite(dr).all() and np.isfinite(di).all() and np.isfinite(ee).all()):
        with np.errstate(all="ignore"):
            out.update(C=complex(np.sum(dr), np.sum(di)), E=float(np.sum(ee)), ok=False, finite=False, abs_c=math.inf, abs_e=math.inf,
                       bound_c=math.inf, bound_e=math.inf)
        return out
    Cr, Ci, E = math.fsum(dr), math.fsum(di), math.fsum(ee)
    ok = False
    if Cr > 0.0 and E > 0.0:
        q = (Cr * Cr + Ci * Ci) / (E * E)
        ok = bool(np.isfinite(q) and q > float(F32(thresh)))
    abs_c, abs_e = math.fsum(np.abs(dr)) + math.fsum(np.abs(di)), math.fsum(np.abs(ee))
    out.update(C=complex(Cr, Ci), E=E, ok=ok, finite=True, abs_c=abs_c, abs_e=abs_e, bound_c=n * U53 * abs_c, bound_e=n * U53 * abs_e)
    return out


class ExactTrk:
    """a TrkModel whose slice carries fcch_exact's records (C, E, ok, bound_*, and finite, abs_*, terms); everything else is
    the TrkModel's, which is not changed.  The update that follows reads these records."""

    def __init__(self, model):
        self.__dict__["m"] = model

    def __getattr__(self, key):
        return getattr(self.__dict__["m"], key)

    def __setattr__(self, key, value):
        setattr(self.__dict__["m"], key, value)

    def slice(self, streams, n0, fn, n_frames):
        m = self.m
        locked = list(m.locked)
        cells, status, rec = m.slice(streams, n0, fn, n_frames)
        for p, rs in enumerate(rec):
            if not rs:
                continue
            frames = [f for f in range(n_frames) if ((fn + f) % HYPER) % 51 in ltm.FCCH_T3]
            assert len(frames) == len(rs)
            for f, r in zip(frames, rs):
                if locked[p]:
                    r.update(fcch_exact(cells[m.c0[p]][8 * f], m.sps, m.fcch_thresh))
                else:
                    r.update(finite=True, abs_c=0.0, abs_e=0.0, bound_c=0.0, bound_e=0.0, n=142 * m.sps,
                             terms=(np.zeros(1), np.zeros(1), np.zeros(1)))
        return cells, status, rec


def record_error(r, C, E):
    """(|exact C - C|, |exact E - E|) of a finite record r, formed from the terms with one rounding"""
    dr, di, ee = r["terms"]
    return (math.hypot(math.fsum(list(dr) + [-C.real]), math.fsum(list(di) + [-C.imag])), abs(math.fsum(list(ee) + [-E])))


# ---- streams ------------------------------------------------------------------------------------------------------------
def noise32(rng, shape, amp):
    out = np.empty(shape, np.complex64)
    out.real = rng.standard_normal(shape, dtype=F32)
    out.imag = rng.standard_normal(shape, dtype=F32)
    return out * F32(amp)


def residual_tone(k, sps, step, residual, amp=3.0):
    """amp exp(2 pi j (k (1/4 + residual) / sps - k step 2^-32)) at stream indices k: an NCO of that step, whatever its phase,
    brings it back to a quarter turn per symbol and `residual` cycle / symbol more"""
    k = np.asarray(k, np.int64)
    turn = ((k.astype(np.uint64) * np.uint64(step)) & np.uint64(M32)).astype(np.float64) / 2.0 ** 32
    return (amp * np.exp(2j * np.pi * (k * (0.25 + residual) / sps - turn))).astype(np.complex64)


def member(x, phone, c0, anchors, n0, fn, F, max_frames=None, **more):
    x = np.ascontiguousarray(x, np.complex64)
    x.setflags(write=False)
    return dict(x=x, phone=list(phone), c0=list(c0), anchors=list(anchors), n0=n0, fn=fn, F=F, max_frames=max_frames or F,
                kw=more.pop("kw", {}), **more)


def apply(mb, *objs):
    for a in mb["anchors"]:
        for o in objs:
            o.set(*a)


# ---- the grid-stride loop -----------------------------------------------------------------------------------------------
def loop_member(sps, n_cols, F=11):
    """see the module's docstring.  promise[p]: the two records' ok flags, None for a phone without a C0 column"""
    gx = TRK_WG // n_cols
    # if the kernel's grid rule changes, these say that the member no longer does its job
    assert 8 * F > gx, "every workgroup forms one cell only: the loop does not go round"
    assert 80 % gx == 0, "the two FCCH cells (t = 0 and 80) fall to different workgroups"
    assert grid_x(n_cols, F) == gx
    frame = 1250 * sps
    n, n0, fn = F * frame + 48, 10 ** 7, 51 * 4321
    P = n_cols // 3
    phone = [min(c // 3, P - 1) for c in range(n_cols)]
    c0 = [-1 if p % 11 == 5 else 3 * p for p in range(P)]
    unlocked = (7, P - 3)
    assert all(c0[p] >= 0 for p in unlocked)
    rng = np.random.default_rng(7000 + 10 * n_cols + sps)
    x = noise32(rng, (n_cols, n), 0.05)
    anchors, promise = [], []
    for p in range(P):
        off, step, phase = int(rng.integers(0, 41)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        d = p % 3 - 1                                          # the anchor a frame behind, on, a frame ahead of the call
        anchors.append((p, int(p not in unlocked), (fn + d) % HYPER, n0 + off + d * frame, step, phase))
        if c0[p] < 0:
            promise.append(None)
            continue
        for f, is_tone in ((0, p % 2 == 0), (10, p % 2 == 1)):
            k = off + f * frame + np.arange(157 * sps)
            if is_tone:
                x[c0[p], k] += residual_tone(k, sps, step, 0.003)
            else:
                x[c0[p], k] = noise32(rng, len(k), 3.0 / np.sqrt(2.0))
        promise.append([False, False] if p in unlocked else [p % 2 == 0, p % 2 == 1])
    return member(x, phone, c0, anchors, n0, fn, F, promise=promise, unlocked=unlocked, gx=gx)


def loop_reuse(sps):
    return loop_member(sps, 204)


def loop_three():
    return loop_member(1, 400)


# ---- lattice cells ------------------------------------------------------------------------------------------------------
LATTICE_OFF = 5


def _cell_member(cell, sps, **more):
    """one column, one phone, one frame from a frame with FN % 51 == 0; the TN 0 cell is `cell`, step 0 and phase 0"""
    n = 1250 * sps + 16
    x = np.zeros((1, n), np.complex64)
    x[0, LATTICE_OFF:LATTICE_OFF + len(cell)] = cell
    x[0, LATTICE_OFF + 157 * sps:] = af.tone(n - LATTICE_OFF - 157 * sps, sps)      # (the other seven cells: the plain tone)
    return member(x, [0], [0], [(0, 1, 51 * 900, 3000 + LATTICE_OFF, 0, 0)], 3000, 51 * 900, 1, cell=np.array(cell, np.complex64), **more)


def straddle(q):
    """the adjacent float32 values lo < q <= hi: ok (q > thresh) is True with lo and False with hi"""
    f = F32(q)
    if float(f) < q:
        return f, np.nextafter(f, F32(np.inf))
    return np.nextafter(f, F32(0)), f


def lattice(sps):
    """[member]: name, expect (C, E, ok at the default threshold where the description promises them), pairs [(lo, hi)]"""
    L, N = 142 * sps, 157 * sps
    out = []
    out.append(_cell_member(af.tone(N, sps), sps, name="plateau", expect=dict(C=L + 0j, E=float(L), ok=True),
                            pairs=[(np.nextafter(F32(1), F32(0)), F32(1))]))
    for name, step, C in (("constant", 0, -1j * L), ("alternating", 2, 1j * L), ("reversed tone", 3, -L + 0j)):
        out.append(_cell_member(af.tone(N, sps, step), sps, name="border " + name, expect=dict(C=C, E=float(L), ok=False), pairs=[]))
    # mixed: symbols 3 .. 70 at 2^10, 71 .. 73 silent, 74 .. 146 at 2^-10, both runs the tone
    amp = np.zeros(157, F32)
    amp[3:71], amp[74:147] = 2.0 ** 10, 2.0 ** -10
    cell = af.tone(N, sps) * np.repeat(amp, sps)
    Cm = sps * (67 * 2.0 ** 20 + 71 * 2.0 ** -20)              # a term per pair of neighbours inside a run (n stops at 145 sps - 1)
    Em = sps * (67.5 * 2.0 ** 20 + 71.5 * 2.0 ** -20)          # a run's end inside the span counts half
    out.append(_cell_member(cell, sps, name="mixed", expect=dict(C=Cm + 0j, E=Em, ok=True), pairs=[straddle(Cm * Cm / (Em * Em))]))
    x, p = af.threshold_stream(sps)
    cell = np.zeros(N, np.complex64)
    cell[3 * sps:3 * sps + L + sps] = x[p:p + L + sps]
    C = float(L - 10 * sps)
    out.append(_cell_member(cell, sps, name="threshold", expect=dict(C=C + 0j, E=float(L), ok=True), pairs=[straddle(C * C / (float(L) * L))]))
    return out


def lattice_check(terms):
    """the lattice condition on a record's terms: multiples of 2^-21 (half the quietest product), the magnitudes summing below 2^53 granules, so that a
    float64 sum in any order is exact"""
    for v in terms:
        g = v * 2.0 ** 21
        assert (g == np.rint(g)).all() and sum(abs(int(t)) for t in g) < 2 ** 53
    return True


def overflow(sps):
    """[member]: the tone at 3e19 and at 1e-23; expect E"""
    out = []
    for name, amp, E in (("3e19", 3e19, math.inf), ("1e-23", 1e-23, 0.0)):
        t = af.tone(157 * sps, sps)
        cell = np.empty(157 * sps, np.complex64)
        cell.real, cell.imag = t.real * F32(amp), t.imag * F32(amp)
        out.append(_cell_member(cell, sps, name=name, expect=dict(E=E)))
    return out


# ---- NaN and Inf inside a stream ----------------------------------------------------------------------------------------
# (word, the component it goes into)
KINDS = ((0x7fc00000, 0), (0xffc00000, 0), (0x7fc00000, 1), (0xffc00000, 1), (0x7f800000, 0), (0xff800000, 0), (0x7f800000, 1), (0xff800000, 1))


def nonfinite(o, variant):
    """2 columns (phone 0: step 0, phase 0x12345678; phone 1: a step), 2 frames from a frame with FN % 51 == 0.  In each column
    every kind once at the first sample of a cell (cell 1 + kind), once at the last (cell 8 + kind), once inside (cell 4 + kind),
    and kind `variant` (column 0) and variant + 4 (column 1) inside the frequency burst's measured span.  The other component
    of such a sample is the noise's.  An infinite sample meets no rotator component that is zero (0 Inf would be a NaN the
    hardware makes up, whose sign is nobody's promise).  places: [(c, t, i, kind)]"""
    sps = o.sps
    frame, F = 1250 * sps, 2
    n, n0, fn = F * frame + 40, 1000, 51 * 77
    rng = np.random.default_rng(7700 + sps)
    x = noise32(rng, (2, n), 1.0)
    w = x.view(np.uint32).reshape(2, n, 2)
    offs, steps, phases = (9, 21), (0, 0x00abcdef), (0x12345678, 0x9e3779b9)
    places = []
    for c in range(2):
        for kind in range(8):
            places += [(c, 1 + kind, 0, kind), (c, 8 + kind, ltm.am.cell_len(8 + kind, sps) - 1, kind), (c, 4 + kind, 40 + 7 * kind, kind)]
        places.append((c, 0, 3 * sps + 61 * sps + 1, (variant + 4 * c) % 8))
    assert len({(c, t, i) for c, t, i, _ in places}) == len(places)
    for c, t, i, kind in places:
        s = ltm.cell_start(t, sps) + i
        w[c, offs[c] + s, KINDS[kind][1]] = KINDS[kind][0]
        rot = ltm.expj_many(o, [((phases[c] + s * steps[c]) & M32) >> 8])[0]
        assert rot.real != 0 and rot.imag != 0
    anchors = [(c, 1, fn, n0 + offs[c], steps[c], phases[c]) for c in range(2)]
    return member(x, [0, 1], [0, 1], anchors, n0, fn, F, places=places)


# ---- the records' capacity ----------------------------------------------------------------------------------------------
def capacity():
    """[member] at sps 1, one column: (max_frames, FN % 51 of the call, the frames f of the call that hold a frequency burst);
    burst j is the exact tone at amplitude j + 1 over a little noise, so no two records are alike"""
    out = []
    for mf, a0, frames in ((52, 40, (0, 11, 21, 31, 41, 51)), (41, 0, (0, 10, 20, 30, 40)), (21, 41, (10, 20))):
        assert frames == tuple(f for f in range(mf) if (a0 + f) % 51 in ltm.FCCH_T3)
        rng = np.random.default_rng(7800 + mf)
        n, n0, fn = mf * 1250 + 20, 500, 51 * 3000 + a0
        x = noise32(rng, (1, n), 0.01)
        for j, f in enumerate(frames):
            x[0, 6 + f * 1250:6 + f * 1250 + 157] += af.tone(157, 1) * F32(j + 1)
        out.append(member(x, [0], [0], [(0, 1, fn, n0 + 6, 0, 0)], n0, fn, mf, frames=frames, cap=mf // 10 + 1))
    return out


# ---- many phones --------------------------------------------------------------------------------------------------------
def many_phones(sps):
    """200 phones, columns 0 and 1 on phone 0 and column 2 on phone 199; ten phones unlocked; acq / src: a search's result on
    5 streams and the sources: phone 63 a valid stream, 64 none (-1), 127 a stream that does not exist (5), 128 a stream whose
    state is not 15, 199 a valid stream whose RFN is the hyperframe's last; the other phones draw from all of these"""
    P, frame = 200, 1250 * sps
    rng = np.random.default_rng(7900 + sps)
    fn = 4
    unlocked = tuple(range(9, 190, 19))                        # 9, 28, ..., 180: ten of them
    assert len(unlocked) == 10 and not {0, 63, 64, 127, 128, 199} & set(unlocked)
    acq = dict(state=np.array([15, 7, 15, 15, 0], np.uint8), sch_w0=np.array([5000, 1, 70000, 20000, 9], np.int32),
               sch_toa=np.array([12.5, 0, -3.75, 0.49999997, 1], np.float32), omega=np.array([0.03, 0, -0.0314159, 3.1415927, 1], np.float32),
               rfn=np.array([77, 5, 2000000, HYPER - 1, 3], np.int32))
    src = rng.choice(np.array([-1, -1, 5, 0, 1, 2, 3, 4, -9], np.int32), P)
    src[[0, 63, 64, 127, 128, 199]] = [-1, 0, -1, 5, 1, 3]
    # phone 199 after the seed: fn 0, pos = 20000 + 1250 sps; moved to the call's frame it starts 7 samples into the buffer
    n0 = 20000 + frame + fn * frame - 7
    anchors = []
    for p in range(P):
        d = int(rng.integers(-100, 101))
        anchors.append((p, int(p not in unlocked), (fn + d) % HYPER, n0 + int(rng.integers(0, 30)) + d * frame, int(rng.integers(0, 1 << 32)),
                        int(rng.integers(0, 1 << 32))))
    x = noise32(rng, (3, frame + 40), 1.0)
    return member(x, [0, 0, 199], [0] + [-1] * 198 + [2], anchors, n0, fn, 1, acq=acq, src=src, unlocked=unlocked)


# ---- update's integer rules ---------------------------------------------------------------------------------------------
def update_edges(sps, F):
    """One column per phone (the last phone has none), toa_gate 2^24, no C0 column.  rows: (t, c, valid, toa) for group_result
    over T = 8 F slots; expect[p]: dict of what the description promises (S, N, adj).  F = 9 puts rows beyond slot 63 and gives
    the phone of the many rows N = 60; F = 1 gives it 8."""
    T = 8 * F
    q = lambda v: F32(v * sps / 256.0)                         # the TOA whose toa 256 / sps is v (exact)
    rows, expect = [], []
    slot = lambda i: (7 * i + 3) % T if F == 1 else 8 + (13 * i + 5) % (T - 8)

    def phone(entries, **e):
        c = len(expect)
        for i, (v, valid) in enumerate(entries):
            rows.append((slot(c + 5 * i), c, valid, v))
        expect.append(e)
    # llrint ties: k + 0.5 for even and odd k, both signs -> round half to even
    for v, r in ((0.5, 0), (1.5, 2), (2.5, 2), (3.5, 4), (-0.5, 0), (-1.5, -2), (-2.5, -2), (-3.5, -4)):
        phone([(q(v), 1)], S=r, N=1)
    # S sps / (256 N) at exact halves, N = 2
    for half, adj in ((-1.5, -1), (-0.5, 0), (0.5, 1), (1.5, 2)):
        S = int(half * 512) // sps
        assert S * sps == half * 512
        phone([(q(S - 3), 1), (q(3), 1)], S=S, N=2, adj=adj)
    # the widest gate: +-2^24 kept, the next float32 beyond it dropped
    for s in (1, -1):
        edge = F32(s * 65536.0 * sps)
        beyond = np.nextafter(edge, F32(s * np.inf))
        assert float(edge) * (256 // sps) == s * 2.0 ** 24 and abs(float(beyond)) * (256 // sps) == 2.0 ** 24 + 2
        phone([(edge, 1), (beyond, 1)], S=s * 2 ** 24, N=1, adj=ltm.timing_adj(s * 2 ** 24, 1, sps))
    # many rows at -2^24: the restoring division on a numerator of -2^31 sps and more
    many = 60 if F == 9 else 8
    c = len(expect)
    for t in range(T - many, T):
        rows.append((t, c, 1, F32(-65536.0 * sps)))
    expect.append(dict(S=-many * 2 ** 24, N=many, adj=ltm.timing_adj(-many * 2 ** 24, many, sps)))
    n_cols = len(expect)
    expect.append(dict(S=0, N=0, adj=0))                       # a phone with no column
    assert len({(t, c) for t, c, _, _ in rows}) == len(rows)
    return dict(rows=rows, expect=expect, n_cols=n_cols, phone=list(range(n_cols)), c0=[-1] * (n_cols + 1), T=T)


def afc_case(sps):
    """2 phones, 2 C0 columns, one frame from a frame with FN % 51 == 0: phone 0 hears the tone with +3e-3 cycle / symbol left
    over (delta < 0), phone 1 with -3e-3 (delta > 0)"""
    frame = 1250 * sps
    rng = np.random.default_rng(8100 + sps)
    n, n0, fn = frame + 32, 0, 51 * 321
    x = noise32(rng, (2, n), 0.05)
    steps = (0x02345678, 0xfedc0000)
    for c, res in enumerate((0.003, -0.003)):
        x[c] += residual_tone(np.arange(n), sps, steps[c], res)
    anchors = [(c, 1, fn, 16 - 9 * c, steps[c], 77 * c) for c in range(2)]
    return member(x, [0, 1], [0, 1], anchors, n0, fn, 1, sign=(-1, 1))
