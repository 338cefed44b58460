"""The census of the schedule family for the Transceiver group's state-machine replay (tests/replay_family.py), on the CPU: the
atoms are what they are meant to be, the scalar model equals oracle/transceiver_model.py fed the same bursts through the CPU oracle,
the call plans hold every switch of the launcher, and -- from the scalar model's record alone -- every regime the family is written
for is really reached, by the kind written for it, in both plans.  tests/test_gpu_replay_family.py then holds the kernels to the
scalar model; a regime this census does not find is one those tests do not grade.

The counts are conditions, not measurements: each is a small fraction of what the committed seeds give (printed with -s)."""
import math
import types

import numpy as np
import pytest

import oraclebind
import replay_family as rf
import transceiver_model as tm

# condition -> ({kind: least count}, plans it is asked of).  A kind named here is the kind WRITTEN for the regime; other kinds reach many
# of them too and are not counted.
BOTH, B_ONLY, A_ONLY = ("A", "B"), ("B",), ("A",)
REQUIRED = {
    "floor0_pass": ({"a_floor": 2000, "a_floor_mixed": 1000}, BOTH),
    "floor0_false_detection": ({"a_floor": 300, "a_floor_mixed": 150}, BOTH),
    "floor0_avg0": ({"a_floor": 300, "a_floor_mixed": 150}, BOTH),
    "fraction_floored_by_success": ({"a_floor": 300, "a_floor_mixed": 150}, BOTH),
    "negative_success": ({"e_negative": 10, "e_negative_mixed": 10}, BOTH),
    "negative_false_detection": ({"e_negative": 10, "e_negative_mixed": 10}, BOTH),
    "negative_decrement": ({"e_negative": 10, "e_negative_mixed": 10}, BOTH),
    "avg_eq_thr2": ({"b_boundary": 400}, BOTH),
    "avg_next_above_thr2": ({"b_boundary": 200}, BOTH),
    "avg_next_below_thr2": ({"b_boundary": 400}, BOTH),
    "quiet_d50_no_decrement": ({"d_quiet_tn": 8, "d_quiet_II": 8, "d_quiet_mixed": 8}, BOTH),
    "quiet_d51_decrement": ({"d_quiet_tn": 8, "d_quiet_mixed": 8}, BOTH),      # (combination II: 51 frames after a mark on an even frame is an idle one)
    "quiet_d52_decrement": ({"d_quiet_tn": 8, "d_quiet_II": 8, "d_quiet_mixed": 8}, BOTH),
    "quiet_decrement_across_wrap": ({"d_quiet_tn": 4, "d_quiet_II": 4, "d_quiet_mixed": 4}, A_ONLY),   # (plan A crosses the hyperframe wrap)
    "detected_under_threshold": ({"c_under": 2000}, BOTH),
    # the clock only runs ahead of the bursts where the frame number steps back: plan A's time is monotonic
    "giant_success": ({"f_giant": 200}, B_ONLY),
    "giant_decrement": ({"f_giant": 30}, B_ONLY),
    "threshold_inf": ({"f_giant": 500}, B_ONLY),
    "clock_ahead_false_detection": ({"f_giant": 8}, B_ONLY),
    "all16_boundaries_differ_seg32": ({"g_chain": 8, "g_chain_ends": 4}, BOTH),
    "all16_boundaries_differ_seg64": ({"g_chain": 8, "g_chain_ends": 4}, BOTH),
    "event_lane0": ({"g_chain": 200, "g_chain_ends": 200}, BOTH),
    "event_lane31": ({"g_chain": 200}, BOTH),
    "event_lane32": ({"g_chain": 50}, BOTH),
    "event_lane63": ({"g_chain": 50, "g_chain_ends": 50}, BOTH),
    "empty_segment_between_busy": ({"h_gaps": 50}, BOTH),
    "cache_age50_kept": ({"i_cache": 20}, BOTH),
    "cache_age51_estimates": ({"i_cache": 20}, BOTH),
    "cache_drop_by_miss": ({"i_cache": 50, "i_cache_V": 30}, BOTH),
    "cache_drop_by_access_burst": ({"i_cache_V": 100}, BOTH),
}


def test_atoms_are_what_they_are_meant_to_be():
    A = rf.atoms()
    avg = lambda n: A.avg[A.ix[n]]
    own = lambda n, tsc: A.det_tsc[A.ix[n], :, tsc]
    assert A.x.size == len(A.names) * rf.CELL and len(A.names) < 64
    assert np.all(avg("zero") == 0.0)
    for tsc in rf.TSCS:
        for n in ("clean%d", "two%d", "faint%d", "faint2_%d") + tuple("giant%d_%%d" % e for e in rf.GIANT_EXP):
            assert own(n % tsc, tsc).all(), n % tsc                       # detected at either length, whatever the power of two
        assert np.all(avg("clean%d" % tsc) > 900.0 ** 2) and np.all(avg("faint%d" % tsc) < 1.0) and np.all(avg("faint%d" % tsc) > 0.0)
        # scaling by a power of two scales avgPwr exactly
        assert np.all(avg("faint%d" % tsc) * np.float32(2048.0 ** 2) == avg("clean%d" % tsc))
        for e in rf.GIANT_EXP:
            assert np.all(avg("giant%d_%d" % (e, tsc)) == avg("faint%d" % tsc) * np.float32(2.0 ** (2 * e + 2)))
            assert np.all(avg("giant%d_%d" % (e, tsc)) > np.float32(2.0 ** 106)) and np.all(np.isfinite(avg("giant%d_%d" % (e, tsc))))
        assert not np.array_equal(A.cells[A.ix["clean%d" % tsc]], A.cells[A.ix["two%d" % tsc]])
    for n in ("rach0", "rach1", "rach2", "rachfaint"):
        assert A.det_rach[A.ix[n]].all(), n
    assert np.all(avg("rachfaint") < 1.0)
    for n in ("noise0", "noise1", "noise2", "noise3", "noisefaint") + tuple("giantnoise%d" % e for e in rf.GIANT_EXP) + ("zero",):
        assert not A.det_rach[A.ix[n]].any() and not A.det_tsc[A.ix[n]][:, list(rf.TSCS)].any(), n
    assert np.all(avg("noisefaint") < 0.1) and np.all(avg("noisefaint") > 0.0)
    for e in rf.GIANT_EXP:
        assert np.all(avg("giantnoise%d" % e) > np.float32(2.0 ** 106))
    # the boundary cells: the oracle's avgPwr is the intended float, P itself or its nearest reachable neighbour on the right side
    for thr in rf.EDGE_THR:
        P = np.float32(thr) * np.float32(thr)
        for side, s in ((-1, "m"), (0, "0"), (1, "p")):
            n = "edge%d%s" % (thr, s)
            assert np.all(avg(n) == A.intended[n]), (n, avg(n), A.intended[n])
            assert not A.det_rach[A.ix[n]].any() and not A.det_tsc[A.ix[n]][:, list(rf.TSCS)].any(), n
        assert A.intended["edge%d0" % thr] == P
        up, dn = A.intended["edge%dp" % thr], A.intended["edge%dm" % thr]
        assert P < up <= np.nextafter(np.nextafter(P, np.float32(np.inf)), np.float32(np.inf))
        assert P > dn >= np.nextafter(np.nextafter(P, np.float32(-np.inf)), np.float32(-np.inf))


def test_call_plans_hold_every_switch():
    a, b = rf.plan_a(), rf.plan_b()
    assert sorted(c[2] for c in a.calls) == sorted(rf.PLAN_A_SIZES)
    assert set(c[1] for c in a.calls) == set(range(8))                 # the calls start on every timeslot number
    fa = a.fn.astype(np.int64)
    steps = np.diff(fa)
    assert set(np.unique(steps)) <= {0, 1, 1 - rf.HYPER} and (steps == 1 - rf.HYPER).sum() == 1      # monotonic, across the wrap once
    jumps = []
    for (f0, t0, n0), (f1, t1, n1) in zip(b.calls[:-1], b.calls[1:]):
        fe, te = rf._after(f0, t0, n0)
        assert te == t1
        jumps.append(tm.fn_delta(f1, fe))
    back = sorted(-j for j in jumps if -1000 < j < 0)
    assert back == list(range(1, 41)) + list(range(708, 713))
    assert {rf.HALF - 1, rf.HALF + 1, rf.HALF} <= {j % rf.HYPER for j in jumps}
    sizes = [c[2] for c in b.calls]
    assert {511, 512, 1023, 1024}.issubset(sizes) and max(sizes) > 1024 and min(sizes) == 1
    for p in (a, b):
        assert 5000 < p.n < 12000
    # every slot configuration occurs, single active timeslots among them
    combs = set()
    single = 0
    for s in range(rf.S):
        _, slots = rf.slot_config(s)
        combs |= set(slots.values())
        single += len(slots) == 1
        if len(slots) < 8:
            combs.add(tm.NONE)
    assert {tm.I, tm.II, tm.IV, tm.V, tm.VII, tm.NONE} <= combs and single >= 16


@pytest.mark.parametrize("plan", ["A", "B"])
def test_family_reaches_every_regime(plan):
    r = rf.run(plan)
    c = rf.census(r)
    missed = []
    for name, (per_kind, plans) in REQUIRED.items():
        for kind, least in per_kind.items():
            got = c[name].get(kind, 0)
            print("plan %s %-32s %-18s %7d (>= %d%s)" % (plan, name, kind, got, least, "" if plan in plans else ", not asked of this plan"))
            if plan in plans and got < least:
                missed.append((name, kind, got, least))
    assert not missed, "regimes the kinds written for them do not reach (condition, kind, got, least): %r" % missed
    # (d) on each timeslot number: every ARFCN of d_quiet_tn has its single timeslot on another number
    k = rf.KINDS.index("d_quiet_tn")
    for a in range(8 * k, 8 * k + 8):
        assert list(rf.slot_config(a)[1]) == [a % 8]
        assert ((r.what[:, a] == 2) & (r.d[:, a] == 51)).sum() >= 1 and ((r.what[:, a] == 1) & (r.d[:, a] == 50)).sum() >= 1, a
    # the thresholds the family is about: the floor, fractions, negatives; and in plan B the range the kernel's 2^52 branch is for
    t = r.thr_after[~np.isnan(r.thr_after)]
    assert (t == 0.0).sum() > 50000 and ((t > 0) & (t < 1)).sum() > 1000 and (t < 0).sum() > 100
    if plan == "B":
        assert ((t >= 2.0 ** 53) & (t < 2.0 ** 60)).sum() > 500 and np.isinf(t).sum() > 500 and not np.isnan(r.final_thr).any()


def test_schedules_replay_without_the_policy():
    """The record run() leaves is the scalar model's answer to the STORED schedule: a second pass over the atoms alone gives it again."""
    for plan in ("A", "B"):
        r = rf.run(plan)
        for a in range(0, rf.S, 5):
            for t, valid, thr in rf.replay_scalar(r, a):
                assert valid == r.valid[t, a] and (thr == r.thr_after[t, a]), (plan, a, t)


@pytest.mark.parametrize("plan,leg_dfe", [("A", True), ("A", False), ("B", True), ("B", False)])
def test_scalar_model_equals_the_transceiver_model(plan, leg_dfe, monkeypatch):
    """oracle/transceiver_model.py (the line-by-line restatement of Transceiver.cpp) fed the schedule's bursts through the CPU oracle:
    what comes back and the threshold after every burst, on both TSC legs, for one ARFCN of every kind (the first 2,500 slots of
    plan A, and of plan B its first 1,500 and a stretch with the long back-steps).  The model calls math.exp, which raises where the C
    library returns inf: it gets the family's exp for this test."""
    shim = types.SimpleNamespace(**{k: getattr(math, k) for k in ("sqrt", "log10", "floor", "pow")}, exp=rf.safe_exp)
    monkeypatch.setattr(tm, "math", shim)
    r = rf.run(plan)
    A = rf.atoms()
    o = oraclebind.Oracle(rf.SPS)
    p = r.plan
    spans = [(0, 2500)] if plan == "A" else [(0, 1500), (int(p.first[len(p.calls) // 2]), int(p.first[len(p.calls) // 2]) + 1500)]
    seen = 0
    with np.errstate(over="ignore"):
        for kind in range(len(rf.KINDS)):
            a = 8 * kind + (kind + (0 if leg_dfe else 3)) % 8
            for lo, hi in spans:
                m = tm.TransceiverModel(o, start=p.start, need_dfe=leg_dfe)
                for cmd in rf.control_commands(a):
                    m.control(cmd)
                if lo:                                                   # start the model in the scalar state before the span
                    st = rf.Scalar(p.start[0])
                    _restore(r, a, lo, st)
                    m.energy_threshold, m.prev_false = st.thr, (st.pf, 0)
                    m.est_time = [(f, 0) for f in st.est]
                    # (the taps are not carried over: with an empty cache the model estimates afresh, which moves neither what
                    #  comes back nor the threshold -- the two things compared here)
                for t in range(lo, hi):
                    ai = r.atom[t, a]
                    tn, fn = int(p.tn[t]), int(p.fn[t])
                    x = A.cells[max(ai, 0)][:157 if tn % 4 == 0 else 156]
                    got = m.pull_radio_vector(x, tn, fn)
                    if ai < 0:
                        assert got is None
                        continue
                    assert (got is not None) == bool(r.valid[t, a]), (plan, rf.KINDS[kind], a, t)
                    assert m.energy_threshold == r.thr_after[t, a], (plan, rf.KINDS[kind], a, t, m.energy_threshold, r.thr_after[t, a])
                    seen += 1
    assert seen > 8000


def _restore(r, a, upto, st):
    """The scalar state of ARFCN a before slot `upto`, by replaying the stored schedule."""
    p, A = r.plan, rf.atoms()
    tsc, _ = rf.slot_config(a)
    with np.errstate(over="ignore"):
        for t in range(upto):
            ai = r.atom[t, a]
            if ai < 0:
                continue
            tn = int(p.tn[t]); k = 1 if tn % 4 == 0 else 0
            ct = int(r.ctype[t, a])
            det = bool(A.det_tsc[ai, k, tsc]) if ct == tm.TSC else bool(A.det_rach[ai, k])
            st.step(ct, A.avg[ai, k], det, int(p.fn[t]), tn, t)
