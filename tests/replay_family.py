"""An adversarial family of SCHEDULES for the Transceiver group's state-machine replay (csrc/trxsig_group.hip: k_group_replay,
k_group_replay_seg<8/16>, k_group_replay_wave, k_group_cache, k_group_cache_wave), and the scalar model that says -- from the CPU
oracle's verdicts on a few dozen bursts alone -- what every slot of every schedule must give.  CPU only: no native library but the
oracle is loaded here.

The replay kernels are speculative: segments replayed side by side from guessed start states and validated in a boundary walk, slots
skipped where "nothing can happen", c detected bursts collapsed into one max(thr - c, 0), "50 quiet frames" decided from a
population count, a branch of its own for thresholds >= 2^52.  Random radio traffic reaches next to none of that (the thresholds
hover in the hundreds), so here the traffic is WRITTEN, slot by slot, to steer each ARFCN's state into one regime:

  atoms      a pool of burst cells at one sample per symbol in ONE short sample buffer, addressed by offset and length (many slots
             point at the same cell: trxsig_trxgroup_pull_bursts only reads its source).  Scaled copies are scaled by exact powers of
             two, so the detector's verdict is unchanged and avgPwr scales exactly.  Each atom's (detected as TSC k, detected as an
             access burst, avgPwr) comes from the CPU oracle, once, for the lengths 156 and 157.
  scalar     Transceiver::pullRadioVector's bookkeeping (oracle/transceiver_model.py:157-205, Transceiver.cpp:288-376) restated as
             a step on (corr type, avgPwr, detected, fn, tn): doubles, the float cast of the threshold, exp() that overflows to inf.
  schedules  one per ARFCN, S = 128 = sixteen kinds x eight seeds, each ARFCN with its own slot configuration.  A schedule is
             written in closed loop: the generator carries the scalar state and picks the next atom from it, by the kind's policy.
  plans      A: monotonic time (across the hyperframe wrap) in calls of every length at which trx_launch_group_replay switches
             form, segment length or segment count, starting on every timeslot number; B: the frame number steps BACK between calls
             (1 .. 40 and 708 .. 712 frames: the clock then runs ahead of the bursts, exp(+d) up to inf) and forward by half a
             hyperframe +- 1 (the FNDelta wrap).

Kinds (the letters are the regimes of the family's census, tests/test_replay_family.py):
  a  count down from 250 to the floor of 0 and stay: faint-noise false detections there give +10 exp(-d), d = 0, 1, 2, ..., and the
     fractional results are counted down through 1
  b  constant cells whose avgPwr is EXACTLY thrF*thrF (the compare is strict) for the thresholds 250, 249, 240, 10, 3, and their
     float neighbours, met by that threshold and the ones a step to either side
  c  detected bursts UNDER their threshold inside runs of accepted ones
  d  silences whose first under-threshold burst comes exactly 50, 51, 52 frames after the last mark; on each timeslot number,
     under combination II (every other frame idle), across the hyperframe wrap (plan A wraps)
  e  thresholds below 10 taken through a quiet decrement: negative, then a success, a false detection or another decrement
  f  giant bursts (x 2^54 .. 2^58) behind a giant threshold (plan B: a false detection while the clock runs 35 .. 37 frames ahead;
     708 frames and more: inf)
  g  mis-speculation chains: every 32- and 64-slot segment moves the threshold and none forgets it; events on a segment's first
     and last slot
  h  segments with no active slot at all between busy ones (combination IV / VI: 8 frames OFF in every 10)
  i  the channel cache: clean and two-path bursts alternate in a timeslot; estimates 50 and 51 frames old, a miss, a detected
     access burst on a combination-V slot
  j  a seeded mixture that keeps the threshold wandering between 0 and ~30

Helper module, no tests here (tests/test_replay_family.py holds the census, tests/test_gpu_replay_family.py grades the kernels)."""
import functools
import math

import numpy as np

import oraclebind
import synth
import transceiver_model as tm

SPS = 1
S = 128
SEED = 31415
TSCS = (2, 5, 0, 7)                                  # ARFCN a's training sequence: TSCS[a % 4]
HYPER = tm.HYPERFRAME
HALF = HYPER // 2
EDGE_THR = (250, 249, 240, 10, 3)                    # thresholds whose float square has boundary cells
GIANT_EXP = (54, 56, 58)
TWO52 = 4503599627370496.0
KINDS = ("a_floor", "a_floor_mixed", "b_boundary", "c_under", "d_quiet_tn", "d_quiet_II", "d_quiet_mixed", "e_negative",
         "e_negative_mixed", "f_giant", "g_chain", "g_chain_ends", "h_gaps", "i_cache", "i_cache_V", "j_mixture")
assert len(KINDS) * 8 == S


def safe_exp(x):
    """exp() as the C library gives it: +inf where Python's raises."""
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


# ---------------------------------------------------------------------------------------------------------------------------------
# atoms
# ---------------------------------------------------------------------------------------------------------------------------------
CELL = 160                                           # samples an atom occupies in the buffer (bursts are 156 / 157 long)


class Atoms:
    """x: complex64 [n * CELL]; name -> index; per atom and length (0: 156, 1: 157): avg float32 [n, 2], det_tsc bool [n, 2, 8]
    (only TSCS are filled), det_rach bool [n, 2]."""

    def __init__(self):
        self.names, self.cells, self.intended = [], [], {}

    def add(self, name, v, intended_avg=None):
        c = np.zeros(CELL, np.complex64)
        c[:min(len(v), 157)] = np.asarray(v, np.complex64)[:157]
        self.names.append(name); self.cells.append(c)
        if intended_avg is not None:
            self.intended[name] = np.float32(intended_avg)
        return len(self.names) - 1

    def finish(self, o):
        self.x = np.concatenate(self.cells)
        self.ix = {n: i for i, n in enumerate(self.names)}
        n = len(self.names)
        self.avg = np.zeros((n, 2), np.float32); self.det_tsc = np.zeros((n, 2, 8), bool); self.det_rach = np.zeros((n, 2), bool)
        for i, c in enumerate(self.cells):
            for k, ln in enumerate((156, 157)):
                v = c[:ln]
                self.avg[i, k] = o.energy_detect(v, 20 * SPS, np.float32(0.0))[1]
                for tsc in TSCS:
                    self.det_tsc[i, k, tsc] = o.analyze_traffic(v, tsc, 3.0)["ok"]
                self.det_rach[i, k] = o.detect_rach(v, 5.0)["ok"]
        self.offset = np.arange(n, dtype=np.int32) * CELL
        return self


def _edge_cell(thr, side):
    """A cell whose avgPwr -- ((sum of the first 20 |x|^2, in float, in order) / 20), sigProcLib.cpp:916-931 -- is exactly P =
    float(thr)^2 (side 0: twenty samples thr + 0j; the sums are integers below 2^24 and exact), or the nearest value energy / 20
    can take above (side +1) / below (-1) it.  energy / 20 does not reach every float: energy ~ 20 P has a coarser last place
    relative to its size than P where 20 P crosses a power of two, so the neighbour is nextafter(P) where that is reachable and at
    most two places away otherwise.  Returns (cell, intended avgPwr), the latter from float arithmetic alone."""
    t = np.float32(thr)
    P = t * t
    v = np.full(157, complex(thr, 0.0), np.complex64)
    if side == 0:
        return v, P
    # 19 samples stay; the twentieth's square moves the float sum by whole places of the sum
    e19 = np.float32(0.0)
    for _ in range(19):
        e19 = np.float32(e19 + P)
    want = np.nextafter(P, np.float32(np.inf if side > 0 else -np.inf))
    last = t
    for _ in range(4096):
        last = np.nextafter(last, np.float32(np.inf if side > 0 else -np.inf))
        sq = np.float32(last * last)                                     # norm2 of a real sample
        avg = np.float32(np.float32(e19 + sq) / np.float32(20.0))
        if (side > 0 and avg >= want) or (side < 0 and avg <= want):
            v[19] = complex(last, 0.0)
            return v, avg
    raise AssertionError("no neighbour cell for threshold %r" % thr)


@functools.lru_cache(maxsize=None)
def atoms():
    o = oraclebind.Oracle(SPS)
    rng = np.random.default_rng(SEED)
    A = Atoms()
    A.add("zero", np.zeros(157))
    for tsc in TSCS:
        bits = synth.normal_bits(np.random.default_rng(SEED + tsc), 1, tsc)
        b = synth.modulate(bits, SPS)[0] * np.complex64(np.exp(1j * (0.7 + tsc)))  # unit amplitude, some phase
        two = b.copy()
        two[SPS:] = two[SPS:] + np.complex64(0.35 - 0.2j) * b[:-SPS]
        A.add("clean%d" % tsc, b * np.float32(1024.0))                          # avgPwr ~ 1e6: opens the gate for thresholds in the hundreds
        A.add("two%d" % tsc, two * np.float32(1024.0))
        A.add("faint%d" % tsc, b * np.float32(0.5))                             # detected, avgPwr < 1
        A.add("faint2_%d" % tsc, two * np.float32(0.5))
        for e in GIANT_EXP:
            A.add("giant%d_%d" % (e, tsc), b * np.float32(2.0 ** e))
    for k in range(3):
        rb = synth.rach_bits(np.random.default_rng(SEED + 100 + k), 1)
        r = synth.modulate(rb, SPS)[0] * np.complex64(np.exp(1j * k))
        r = np.concatenate([np.zeros(3 * k, np.complex64), r])[:157]
        A.add("rach%d" % k, r * np.float32(1024.0))
    A.add("rachfaint", r * np.float32(0.5))
    # noise no correlator detects (as any TSC in use or as an access burst, at either length): the first draws that qualify
    got = []
    while len(got) < 4:
        w = ((rng.standard_normal(157) + 1j * rng.standard_normal(157)) / np.sqrt(2.0)).astype(np.complex64)
        if any(o.analyze_traffic(w[:n], t, 3.0)["ok"] for t in TSCS for n in (156, 157)) or any(o.detect_rach(w[:n], 5.0)["ok"] for n in (156, 157)):
            continue
        got.append(w)
    for k, (w, sc) in enumerate(zip(got, (64.0, 512.0, 2048.0, 16384.0))):
        A.add("noise%d" % k, w * np.float32(sc))                                # loud: avgPwr ~ sc^2
    A.add("noisefaint", got[0] * np.float32(0.25))                              # passes the gate only near thr = 0
    for e in GIANT_EXP:
        A.add("giantnoise%d" % e, got[1] * np.float32(2.0 ** e))
    for thr in EDGE_THR:
        for side in (-1, 0, 1):
            v, want = _edge_cell(thr, side)
            A.add("edge%d%s" % (thr, "m0p"[side + 1]), v, intended_avg=want)
    return A.finish(o)


# ---------------------------------------------------------------------------------------------------------------------------------
# slot configurations and call plans
# ---------------------------------------------------------------------------------------------------------------------------------
def slot_config(a):
    """(tsc, {tn: combination}) of ARFCN a = kind * 8 + seed."""
    kind, seed = KINDS[a // 8], a % 8
    tsc = TSCS[a % 4]
    mixed = ({t: tm.I for t in range(8)}, {0: tm.V, 1: tm.VII, 2: tm.I, 3: tm.IV, 5: tm.II}, {1: tm.II, 2: tm.II, 6: tm.I},
             {0: tm.IV, 4: tm.I}, {t: tm.I for t in (1, 3, 5, 7)}, {0: tm.VII, 1: tm.VII, 2: tm.I}, {2: tm.I, 3: tm.I, 4: tm.V},
             {seed: tm.I})
    if kind in ("a_floor", "b_boundary", "c_under", "g_chain", "g_chain_ends", "f_giant"):
        return tsc, {t: tm.I for t in range(8)}
    if kind in ("d_quiet_tn", "e_negative"):
        return tsc, {seed: tm.I}                                         # a single active timeslot, each number in turn
    if kind == "d_quiet_II":
        return tsc, ({seed: tm.II} if seed < 4 else {seed: tm.II, (seed + 3) % 8: tm.II})
    if kind == "h_gaps":
        return tsc, ({seed: tm.IV} if seed < 6 else {0: tm.IV, 3: tm.VI})
    if kind == "i_cache":
        return tsc, ({seed: tm.I} if seed < 4 else {seed: tm.I, 0: tm.VII})
    if kind == "i_cache_V":
        return tsc, ({0: tm.V}, {0: tm.V, 1: tm.I}, {4: tm.V}, {0: tm.V, 2: tm.VII})[seed % 4]
    return tsc, mixed[seed]


def control_commands(a):
    tsc, slots = slot_config(a)
    return ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % tsc] + \
           ["CMD SETSLOT %d %d" % (tn, c) for tn, c in sorted(slots.items())] + ["CMD POWERON"]


def corr_type(comb, fn):
    m = tm.TransceiverModel.__new__(tm.TransceiverModel)
    m.chan_type = [comb]
    return m.expected_corr_type(0, fn)


class Plan:
    """calls: [(fn, tn, n_slots)]; start: the group's start time; fn / tn / call / lane: per slot index of the whole run (call =
    the call's number, lane = the slot's place in its call)."""

    def __init__(self, name, start, calls):
        self.name, self.start, self.calls = name, start, calls
        fn, tn, call, lane = [], [], [], []
        for k, (f, t, n) in enumerate(calls):
            for i in range(n):
                fn.append((f + (t + i) // 8) % HYPER); tn.append((t + i) % 8); call.append(k); lane.append(i)
        self.fn, self.tn, self.call, self.lane = (np.array(v, np.int64) for v in (fn, tn, call, lane))
        self.n = len(fn)
        self.first = np.concatenate([[0], np.cumsum([c[2] for c in calls])[:-1]]).astype(np.int64)


def _after(f, t, n):
    return (f + (t + n) // 8) % HYPER, (t + n) % 8


PLAN_A_SIZES = (1, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 383, 384, 385, 511, 512, 513, 1023, 1024, 1025, 1500)


@functools.lru_cache(maxsize=None)
def plan_a():
    """Monotonic time from 300 frames before the hyperframe wrap: every call length at which the launcher switches (the stepping
    forms below 128 / 384 slots, the wave form's segment length at 512 and its limit at 1,024), in an order (a seeded shuffle, the
    first found) in which the calls start on every timeslot number."""
    rng = np.random.default_rng(SEED)
    for _ in range(1000):
        order = rng.permutation(len(PLAN_A_SIZES))
        sizes = [PLAN_A_SIZES[i] for i in order]
        starts = set(int(v) % 8 for v in 3 + np.concatenate([[0], np.cumsum(sizes)[:-1]]))
        big = sizes.index(1500)
        if len(starts) == 8 and big >= 6:                                # (the long calls not all at the start)
            break
    else:
        raise AssertionError("no order of plan A starts on every timeslot number")
    f, t = HYPER - 300, 3
    start = (f, t)
    calls = []
    for n in sizes:
        calls.append((f, t, n))
        f, t = _after(f, t, n)
    return Plan("A", start, calls)


@functools.lru_cache(maxsize=None)
def plan_b():
    """The frame number jumps between calls.  Each back-step k (1 .. 40 and 708 .. 712 frames, shuffled) is followed by a call during
    which the clock runs ahead of the bursts, then by a forward step that leaves every ARFCN more than 50 frames past its last mark
    (so that its next under-threshold burst re-bases the clock); at the end, forward by half a hyperframe - 1, + 1 and + 0 (the
    FNDelta wrap: the difference to a mark d frames back becomes d + half - 1 -- which wraps negative for d >= 1)."""
    rng = np.random.default_rng(SEED + 1)
    backs = [int(k) for k in rng.permutation(np.concatenate([np.arange(1, 41), np.arange(708, 713)]))]
    ahead = (64, 96, 128, 72, 200, 104, 80, 88, 64, 120)                   # (>= 8 frames: the difference rises through -35 .. -37 after the long steps)
    normal = (33, 8, 65, 1, 40, 24, 7, 129, 16, 50)
    special = {10: 512, 20: 1024, 30: 511, 40: 1023}                    # (sixteen segments of 32 and of 64 slots under this plan too)
    f, t = 123456, 5
    start = (f, t)
    calls = []

    def call(n):
        nonlocal f, t
        calls.append((f, t, n))
        f, t = _after(f, t, n)
    call(200)
    for j, k in enumerate(backs):
        call(special.get(j, normal[j % len(normal)]))
        f = (f - k) % HYPER
        call(ahead[j % len(ahead)])
        f = (f + k + 60) % HYPER
    call(1100)
    for step in (HALF - 1, HALF + 1, HALF):
        f = (f + step) % HYPER
        call(130)
    return Plan("B", start, calls)


# ---------------------------------------------------------------------------------------------------------------------------------
# the scalar model
# ---------------------------------------------------------------------------------------------------------------------------------
class Scalar:
    """One ARFCN's receive state: mEnergyThreshold, prevFalseDetectionTime, and per timeslot channelEstimateTime and which slot of
    the run (its index) estimated the channel the slot's cache holds (None: channelResponse[tn] == NULL)."""
    __slots__ = ("thr", "pf", "est", "src")

    def __init__(self, start_fn):
        self.thr = 250.0; self.pf = start_fn; self.est = [start_fn] * 8; self.src = [None] * 8

    def step(self, ct, avg, det, fn, tn, t):
        """The burst of slot index t: corr type ct (tm.TSC / tm.RACH), avgPwr (float32), the correlator's stateless answer.
        Returns (valid, what, d, estimates, taps): what in "under" / "qdec" / "succ" / "fail"; d = FNDelta to the mark BEFORE the
        step; estimates: this burst estimates the channel (equalising leg); taps: the slot index whose estimate equalises it."""
        thr_f = np.float32(self.thr)
        d = tm.fn_delta(fn, self.pf)
        if not (avg > thr_f * thr_f):                                    # energyDetect (:298), the threshold through a float
            if float(d) > 50:
                self.thr -= 10.0; self.pf = fn
                return False, "qdec", d, False, None
            return False, "under", d, False, None
        estimates = False
        if ct == tm.TSC:
            stale = float(tm.fn_delta(fn, self.est[tn])) > 50 or self.src[tn] is None
            if stale:
                self.src[tn] = None
            if det:
                self.thr -= 1.0
                if self.thr < 0.0:
                    self.thr = 0.0
                if stale:
                    self.src[tn] = t; self.est[tn] = fn; estimates = True
                return True, "succ", d, estimates, self.src[tn]
            self.thr += 10.0 * safe_exp(-float(d)); self.pf = fn; self.src[tn] = None
            return False, "fail", d, False, None
        if det:
            self.thr -= 1.0
            if self.thr < 0.0:
                self.thr = 0.0
            self.src[tn] = None
            return True, "succ", d, False, None
        self.thr += 10.0 * safe_exp(-float(d)); self.pf = fn
        return False, "fail", d, False, None


# ---------------------------------------------------------------------------------------------------------------------------------
# schedules: closed-loop policies
# ---------------------------------------------------------------------------------------------------------------------------------
def _policy(kind, seed, A, tsc):
    """-> choose(state, ct, fn, tn, t, lane, rng, mem) -> atom name.  `mem` is the policy's scratch dict."""
    ok_t, ok_r = "clean%d" % tsc, "rach0"
    loud = lambda st: "noise3" if st.thr > 1500 else ("noise2" if st.thr > 300 else "noise1")

    def succ(ct, rng=None, alt=False):
        if ct == tm.RACH:
            return "rach%d" % (0 if rng is None else rng.integers(0, 3))
        return ("two%d" % tsc) if alt else ok_t

    def faint_det(ct):
        return ("faint%d" % tsc) if ct == tm.TSC else "rachfaint"

    def a_floor(st, ct, fn, tn, t, lane, rng, mem):
        if st.thr == 0.0:
            r = rng.integers(0, 10)
            d = tm.fn_delta(fn, st.pf)
            if r == 0 or (r == 1 and d > 2):
                return "noisefaint"                                      # + 10 exp(-d)
            if r == 2 and d <= 50:
                return "zero"                                            # avgPwr 0 at the floor: never passes
            if r == 3:
                return faint_det(ct)                                     # passes only here
            return succ(ct, rng)
        r = rng.integers(0, 16)
        if r == 0 and st.thr < 40:
            return loud(st)
        if r == 1:
            return faint_det(ct)
        return succ(ct, rng)

    def b_boundary(st, ct, fn, tn, t, lane, rng, mem):
        # at thr == T: the cell of T's square, its neighbour below, last its neighbour above (which passes and moves the threshold);
        # at T + 1: none passes; at T - 1: all would pass, one is sent
        for T in EDGE_THR:
            if st.thr in (T - 1.0, float(T), T + 1.0):
                seq = {0: "0m0mp", 1: "0mp", -1: "m"}[int(st.thr - T)]
                k = mem.get((T, st.thr), 0)
                if k < len(seq):
                    mem[(T, st.thr)] = k + 1
                    return "edge%d%s" % (T, seq[k])
        if st.thr == 0.0:
            if tm.fn_delta(fn, st.pf) == 0 or rng.integers(0, 4) == 0:
                mem.clear()
                return "noise0"                                          # d = 0: + 10 exp(0), exactly 10 again
        return succ(ct)

    def c_under(st, ct, fn, tn, t, lane, rng, mem):
        if st.thr < 3.0:
            mem["bump"] = int(rng.integers(3, 30))
        if mem.get("bump", 0) > 0:
            mem["bump"] -= 1
            return loud(st)
        return faint_det(ct) if rng.integers(0, 10) < 3 else succ(ct, rng)

    def d_quiet(st, ct, fn, tn, t, lane, rng, mem):
        d = tm.fn_delta(fn, st.pf)
        if mem.get("pf") != st.pf:                                       # a new mark: the next silence's target
            mem["pf"] = st.pf
            mem["target"] = (50, 51, 52, 53)[mem.get("k", seed) % 4]; mem["k"] = mem.get("k", seed) + 1
        if st.thr < 120.0 and d <= 1:
            return loud(st)                                              # keep the threshold in the hundreds: + 10 exp(-d)
        if 50 <= d < mem["target"]:
            return succ(ct)                                              # nothing under the threshold before the target frame
        if d >= mem["target"] or rng.integers(0, 8):
            return "zero" if rng.integers(0, 3) else faint_det(ct)
        return succ(ct)

    def e_negative(st, ct, fn, tn, t, lane, rng, mem):
        d = tm.fn_delta(fn, st.pf)
        if st.thr < 0.0:
            r = mem.setdefault("follow", int(rng.integers(0, 3)))
            if r == 0:
                mem.pop("follow"); return succ(ct)                       # floored at 0
            if r == 1:
                mem.pop("follow"); return loud(st)                       # negative + 10 exp(-d)
            if d > 50:
                mem.pop("follow")                                        # another decrement
            return "zero"
        if st.thr >= 10.0 + 1e-9:
            return succ(ct, rng)
        if st.thr == 0.0 and rng.integers(0, 3):
            return "noisefaint" if rng.integers(0, 2) else succ(ct)
        return "zero" if rng.integers(0, 6) else faint_det(ct)           # quiet until the decrement

    def f_giant(st, ct, fn, tn, t, lane, rng, mem):
        d = tm.fn_delta(fn, st.pf)
        want = (-35, -36, -37)[seed % 3] if seed < 6 else None
        if st.thr >= TWO52:
            if seed % 2 and d < -700:
                return "noise3"                                          # + 10 exp(7xx): inf
            r = rng.integers(0, 8)
            e = GIANT_EXP[int(rng.integers(0, 3))]
            if r < 4:
                return "giant%d_%d" % (e, tsc)
            if r == 4:
                return "giantnoise%d" % e
            if r == 5:
                return "zero"
            return succ(ct) if r == 6 else faint_det(ct)
        if t >= 100 * seed and ((want is not None and d == want) or (want is None and d < -700)):
            return "noise3"
        if d < -3:
            return succ(ct) if rng.integers(0, 4) else "zero"
        if st.thr == 0.0:
            return "noisefaint" if rng.integers(0, 6) == 0 else "giant%d_%d" % (GIANT_EXP[int(rng.integers(0, 3))], tsc)
        return succ(ct)

    def g_chain(st, ct, fn, tn, t, lane, rng, mem):
        ends = (0, 31, 32, 63) if kind == "g_chain" else (0, 63)
        if lane % 64 in ends:
            if st.thr > 40.0 and not (seed % 2 and rng.integers(0, 5) == 0):
                return succ(ct)
            return loud(st)
        return "zero" if tm.fn_delta(fn, st.pf) <= 50 or rng.integers(0, 2) else faint_det(ct)

    def h_gaps(st, ct, fn, tn, t, lane, rng, mem):
        r = rng.integers(0, 8)
        if r < 4:
            return succ(ct, rng)
        if r == 4 and st.thr < 60:
            return loud(st)
        return "zero" if r == 5 else ("rachfaint" if r == 6 else succ(ct, rng))

    def i_cache(st, ct, fn, tn, t, lane, rng, mem):
        r = rng.integers(0, 40)
        if r == 0:
            return loud(st)                                              # a miss drops the entry
        if ct == tm.RACH:
            return succ(ct, rng) if r < 30 else "zero"
        if r == 1:
            return "zero"
        return succ(ct, alt=bool((fn + seed * (fn // 7)) & 1))

    def j_mixture(st, ct, fn, tn, t, lane, rng, mem):
        r = rng.integers(0, 10)
        if st.thr < 5.0 and r < 3:
            return "noisefaint" if (st.thr == 0.0 and r == 0) else loud(st)
        if r < 6 or st.thr > 30.0:
            return succ(ct, rng, alt=bool(r & 1))
        return (faint_det(ct), "zero", "noisefaint", loud(st))[r - 6]

    table = dict(a_floor=a_floor, a_floor_mixed=a_floor, b_boundary=b_boundary, c_under=c_under, d_quiet_tn=d_quiet, d_quiet_II=d_quiet,
                 d_quiet_mixed=d_quiet, e_negative=e_negative, e_negative_mixed=e_negative, f_giant=f_giant, g_chain=g_chain,
                 g_chain_ends=g_chain, h_gaps=h_gaps, i_cache=i_cache, i_cache_V=i_cache, j_mixture=j_mixture)
    inner = table[kind]

    def choose(st, ct, fn, tn, t, lane, rng, mem):
        name = inner(st, ct, fn, tn, t, lane, rng, mem)
        # while the clock runs ahead of the bursts a false detection adds 10 exp(+d), which no run of successes takes back: only
        # kind f goes there
        if kind != "f_giant" and tm.fn_delta(fn, st.pf) < -3:
            ai, k = A.ix[name], 1 if tn % 4 == 0 else 0
            det = A.det_tsc[ai, k, tsc] if ct == tm.TSC else A.det_rach[ai, k]
            thr_f = np.float32(st.thr)
            if not det and A.avg[ai, k] > thr_f * thr_f:
                return "zero"
        return name
    return choose


class Run:
    """A plan's schedules and the scalar model's answers.  [n_slots, S] arrays: atom (int32, -1 where no correlator runs), ctype,
    valid, thr_after (NaN where no correlator ran), thr_state (the threshold after the slot, carried through idle slots), what
    (0 none, 1 under, 2 qdec, 3 succ, 4 fail), d, thr_before, est (the burst estimates), taps (slot index whose estimate equalises
    the burst, -1); final_thr [S]."""
    WHAT = {"under": 1, "qdec": 2, "succ": 3, "fail": 4}


@functools.lru_cache(maxsize=None)
def run(plan_name):
    plan = plan_a() if plan_name == "A" else plan_b()
    A = atoms()
    n = plan.n
    r = Run()
    r.plan = plan
    r.atom = np.full((n, S), -1, np.int32); r.ctype = np.zeros((n, S), np.int8); r.valid = np.zeros((n, S), bool)
    r.thr_after = np.full((n, S), np.nan); r.thr_state = np.zeros((n, S)); r.what = np.zeros((n, S), np.int8)
    r.d = np.zeros((n, S), np.int64); r.thr_before = np.full((n, S), np.nan); r.est = np.zeros((n, S), bool)
    r.taps = np.full((n, S), -1, np.int64); r.age = np.full((n, S), -1, np.int64); r.had_entry = np.zeros((n, S), bool)
    r.final_thr = np.zeros(S)
    fn_l, tn_l, lane_l = plan.fn.tolist(), plan.tn.tolist(), plan.lane.tolist()
    mdl = tm.TransceiverModel.__new__(tm.TransceiverModel)
    with np.errstate(over="ignore"):
        for a in range(S):
            kind, seed = KINDS[a // 8], a % 8
            tsc, slots = slot_config(a)
            mdl.chan_type = [slots.get(q, tm.NONE) for q in range(8)]
            choose = _policy(kind, seed, A, tsc)
            rng = np.random.default_rng(SEED + 1000 * a + (0 if plan_name == "A" else 7))
            st = Scalar(plan.start[0])
            mem = {}
            active_tn = [q for q in range(8) if mdl.chan_type[q] != tm.NONE]
            for t in range(n):
                tn = tn_l[t]
                if tn not in active_tn:
                    r.thr_state[t, a] = st.thr
                    continue
                fn = fn_l[t]
                ct = mdl.expected_corr_type(tn, fn)
                r.ctype[t, a] = ct
                if ct in (tm.OFF, tm.IDLE):
                    r.thr_state[t, a] = st.thr
                    continue
                ai = A.ix[choose(st, ct, fn, tn, t, lane_l[t], rng, mem)]
                k = 1 if tn % 4 == 0 else 0
                det = bool(A.det_tsc[ai, k, tsc]) if ct == tm.TSC else bool(A.det_rach[ai, k])
                r.atom[t, a] = ai
                r.thr_before[t, a] = st.thr
                if ct == tm.TSC:
                    r.age[t, a] = tm.fn_delta(fn, st.est[tn])
                r.had_entry[t, a] = st.src[tn] is not None
                valid, what, d, est, taps = st.step(ct, A.avg[ai, k], det, fn, tn, t)
                r.valid[t, a] = valid; r.what[t, a] = Run.WHAT[what]; r.d[t, a] = d; r.est[t, a] = est
                r.taps[t, a] = -1 if taps is None else taps
                r.thr_after[t, a] = st.thr; r.thr_state[t, a] = st.thr
            r.final_thr[a] = st.thr
    return r


def replay_scalar(r, a, upto=None):
    """The scalar model run AGAIN over ARFCN a's stored schedule (no policy in the loop): [(t, valid, thr_after)]."""
    plan, A = r.plan, atoms()
    tsc, _ = slot_config(a)
    st = Scalar(plan.start[0])
    out = []
    with np.errstate(over="ignore"):
        for t in range(plan.n if upto is None else upto):
            ai = r.atom[t, a]
            if ai < 0:
                continue
            tn = int(plan.tn[t]); k = 1 if tn % 4 == 0 else 0
            ct = int(r.ctype[t, a])
            det = bool(A.det_tsc[ai, k, tsc]) if ct == tm.TSC else bool(A.det_rach[ai, k])
            valid = st.step(ct, A.avg[ai, k], det, int(plan.fn[t]), tn, t)[0]
            out.append((t, valid, st.thr))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the census: which regimes a run reaches, from the scalar model's record alone
# ---------------------------------------------------------------------------------------------------------------------------------
def wave_calls(plan):
    """[(call number, first slot, n_slots, segment length, K)] of the calls the wave form takes (n <= 1,024)."""
    out = []
    for k, (f, t, n) in enumerate(plan.calls):
        if n <= 1024:
            seg = 32 if n <= 512 else 64
            out.append((k, int(plan.first[k]), n, seg, (n + seg - 1) // seg))
    return out


def census(r):
    """{condition: {kind: count}} over the run."""
    plan, A = r.plan, atoms()
    kind_of = np.array([a // 8 for a in range(S)])
    act = r.atom >= 0
    avg = np.zeros(r.atom.shape, np.float32)
    k157 = (plan.tn % 4 == 0).astype(int)
    for a in range(S):
        m = act[:, a]
        avg[m, a] = A.avg[r.atom[m, a], k157[m]]
    tb = r.thr_before
    with np.errstate(invalid="ignore", over="ignore"):
        tf = tb.astype(np.float32)
        P = tf * tf
        succ, fail, qdec, under = r.what == 3, r.what == 4, r.what == 2, r.what == 1
        passed = succ | fail
        frac = act & (tb > 0) & (tb < 1)
        cond = {
            "floor0_pass": act & (tb == 0.0) & passed,
            "floor0_false_detection": act & (tb == 0.0) & fail,
            "floor0_avg0": act & (tb == 0.0) & (avg == 0.0),
            "fraction_floored_by_success": frac & succ,
            "negative_success": act & (tb < 0) & succ,
            "negative_false_detection": act & (tb < 0) & fail,
            "negative_decrement": act & (tb < 0) & qdec,
            "avg_eq_thr2": act & (avg == P) & (P > 1),
            "quiet_decrement_across_wrap": qdec & ((plan.fn[:, None] - r.d) < 0) & (r.d > 0),
            "avg_next_above_thr2": act & (avg > P) & (avg <= np.nextafter(np.nextafter(P, np.float32(np.inf)), np.float32(np.inf))),
            "avg_next_below_thr2": act & (avg < P) & (avg >= np.nextafter(np.nextafter(P, np.float32(-np.inf)), np.float32(-np.inf))) & (P > 1),
            "quiet_d50_no_decrement": under & (r.d == 50),
            "quiet_d51_decrement": qdec & (r.d == 51),
            "quiet_d52_decrement": qdec & (r.d == 52),
            "detected_under_threshold": (under | qdec) & _detected(r, A, plan),
            "giant_success": succ & (tb >= TWO52),
            "giant_decrement": qdec & (tb >= TWO52),
            "threshold_inf": act & np.isinf(r.thr_after),
            "clock_ahead_false_detection": fail & (r.d < 0),
            "cache_age50_kept": succ & (r.ctype == tm.TSC) & (r.age == 50) & r.had_entry & ~r.est,
            "cache_age51_estimates": succ & (r.ctype == tm.TSC) & (r.age == 51) & r.had_entry & r.est,
            "cache_drop_by_miss": fail & (r.ctype == tm.TSC) & r.had_entry,
            "cache_drop_by_access_burst": succ & (r.ctype == tm.RACH) & r.had_entry,
        }
    out = {}
    for name, m in cond.items():
        per = np.zeros(len(KINDS), int)
        np.add.at(per, kind_of, m.sum(axis=0))
        out[name] = {KINDS[k]: int(per[k]) for k in range(len(KINDS)) if per[k]}
    # events on a segment's first / last lane, segments without an active slot between busy ones, and calls whose TRUE threshold at
    # the start of every one of 16 segments differs from every other's (each start state the speculation guesses is wrong)
    event = (r.what >= 2)
    lanes = {"event_lane0": {}, "event_lane31": {}, "event_lane32": {}, "event_lane63": {}, "empty_segment_between_busy": {},
             "all16_boundaries_differ_seg32": {}, "all16_boundaries_differ_seg64": {}}

    def bump(key, a, c=1):
        if c:
            lanes[key][KINDS[a // 8]] = lanes[key].get(KINDS[a // 8], 0) + int(c)
    for k, first, n, seg, K in wave_calls(plan):
        ev = event[first:first + n]
        ac = act[first:first + n]
        for ln in (0, 31, 32, 63):
            if ln >= seg:
                continue
            c = ev[ln::seg].sum(axis=0)
            for a in np.flatnonzero(c):
                bump("event_lane%d" % ln, a, c[a])
        busy = np.array([ac[j * seg:(j + 1) * seg].any(axis=0) for j in range(K)])          # [K, S]
        for a in range(S):
            b = busy[:, a]
            if b.any():
                lo, hi = np.flatnonzero(b)[[0, -1]]
                bump("empty_segment_between_busy", a, (~b[lo:hi]).sum())
        if K == 16:
            for a in range(S):
                starts = [r.thr_state[first + j * seg - 1, a] if first + j * seg > 0 else 250.0 for j in range(K)]
                if len(set(starts)) == K:
                    bump("all16_boundaries_differ_seg%d" % seg, a)
    out.update(lanes)
    return out


def _detected(r, A, plan):
    det = np.zeros(r.atom.shape, bool)
    k157 = (plan.tn % 4 == 0).astype(int)
    for a in range(S):
        tsc = TSCS[a % 4]
        m = r.atom[:, a] >= 0
        ai = r.atom[m, a]
        kk = k157[m]
        det[m, a] = np.where(r.ctype[m, a] == tm.TSC, A.det_tsc[ai, kk, tsc], A.det_rach[ai, kk])
    return det


def listed(r, first, n):
    """offset / length int32 [S, n] of the call's bursts as trxsig_trxgroup_pull_bursts takes them (burst t of ARFCN a = entry
    a * n + t).  A slot where no correlator runs lists the all-zero atom: the group does not look at it."""
    A = atoms()
    at = r.atom[first:first + n].T
    off = A.offset[np.where(at >= 0, at, A.ix["zero"])].astype(np.int32)
    ln = np.broadcast_to(np.where(r.plan.tn[first:first + n] % 4 == 0, 157, 156).astype(np.int32), (S, n))
    return np.ascontiguousarray(off), np.ascontiguousarray(ln)
