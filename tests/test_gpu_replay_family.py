"""The Transceiver group's state-machine replay (csrc/trxsig_group.hip) on the adversarial schedule family of
tests/replay_family.py: every kernel form -- k_group_replay, k_group_replay_seg<8/16>, k_group_replay_wave, and on the equalising
leg k_group_cache / k_group_cache_wave -- against the family's scalar model, slot by slot and exactly: what comes back, the threshold
after every burst (double equality; NaN where no correlator ran; inf where the model says inf), the thresholds at the end.  The
schedules reach what radio traffic does not (tests/test_replay_family.py counts it): thresholds on the floor of 0, fractional and
negative ones, avgPwr == thrF^2, silences of exactly 50 / 51 / 52 frames, a clock that runs ahead of the bursts, thresholds of
2^53 .. 2^59 and inf, events on a segment's first and last slot, calls in which every speculated start state is wrong.

The bursts go in through trxsig_trxgroup_pull_bursts, as LISTED bursts: thousands of list entries point at the same few dozen cells
(pull_core only reads its source: the detectors, the channel estimate, the equaliser and the demodulator all take it const).

Each test prints its wall times (pytest -s)."""
import ctypes
import time

import numpy as np
import pytest

import _pkg
import replay_family as rf
import transceiver_model as tm

pytestmark = pytest.mark.gpu

S = rf.S


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def hip():
    h = ctypes.CDLL("libamdhip64.so")
    h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def dev(ptr, n, dtype):                                              # a result's device array -> host
        a = np.empty(n, dtype)
        if n:
            assert h.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0     # hipMemcpyDeviceToHost
        return a
    return dev


@pytest.fixture(scope="module")
def expected():
    """Per plan: the scalar model's run, each active cell's oracle verdict and avgPwr."""
    cache = {}

    def get(plan):
        if plan not in cache:
            r = rf.run(plan)
            A = rf.atoms()
            det = rf._detected(r, A, r.plan)
            k157 = (r.plan.tn % 4 == 0).astype(int)
            avg = np.zeros(r.atom.shape, np.float32)
            for a in range(S):
                m = r.atom[:, a] >= 0
                avg[m, a] = A.avg[r.atom[m, a], k157[m]]
            cache[plan] = (r, det, avg)
        return cache[plan]
    return get


def run_group(pkg, hip, leg, plan_name, expected, soft_of=None, keep_soft=True):
    """The whole plan through one group, call by call; every call checked against the scalar model as it is collected.  Returns
    valid / rssi / timing / threshold [n_slots, S], the soft bits of the valid cells (in (slot, ARFCN) order; of the ARFCN columns
    soft_of only, [n_slots, len(soft_of), 148], if given) and the thresholds at the end."""
    import torch
    r, det, avg = expected(plan_name)
    plan, A = r.plan, rf.atoms()
    ctx = pkg.TrxSig(rf.SPS, 0)
    ctx.use_torch_stream()
    g = pkg.TrxGroup(ctx, S, tsc_leg=leg, start=plan.start)
    for a in range(S):
        for cmd in rf.control_commands(a):
            assert g.control(a, cmd).split()[:3] == ["RSP", cmd.split()[1], "0"], (a, cmd)
    dx = torch.from_numpy(A.x.view(np.float32)).to("cuda:0")
    out = dict(valid=np.zeros((plan.n, S), bool), rssi=np.zeros((plan.n, S), np.int32), timing=np.zeros((plan.n, S), np.int32),
               threshold=np.zeros((plan.n, S)))
    softs = []
    for k, (fn, tn, n) in enumerate(plan.calls):
        lo = int(plan.first[k])
        off, ln = rf.listed(r, lo, n)
        d_off, d_len = torch.from_numpy(off).to("cuda:0"), torch.from_numpy(ln).to("cuda:0")
        res = g.pull_bursts(dx, d_off, d_len, n, fn, tn)
        assert res.n_slots == n and res.n_arfcn == S
        c = g.collect(soft=keep_soft)                                    # (raises if a time-parallel replay hit its round bound)
        where = (plan_name, leg, "call %d: %d slots from (%d, %d)" % (k, n, fn, tn))
        # the stateless detectors' answers are the atoms' oracle values
        row = hip(res.d_row, n * S, np.int32).reshape(n, S)
        act = r.atom[lo:lo + n] >= 0
        assert np.array_equal(row >= 0, act), where
        assert res.n_rows == act.sum(), where
        flags, pw = hip(res.d_flags, res.n_rows, np.uint8), hip(res.d_avgpwr, res.n_rows, np.float32)
        assert not (flags & 128).any(), where                            # TRXSIG_F_BADLEN
        assert np.array_equal((flags[row[act]] & pkg.F_DETECT) != 0, det[lo:lo + n][act]), where
        assert np.array_equal(pw[row[act]], avg[lo:lo + n][act]), where
        # the state machine: what comes back and the threshold after every burst
        bad = np.argwhere(c["valid"] != r.valid[lo:lo + n])
        assert not len(bad), where + ("valid, first at (slot, ARFCN)", bad[0], rf.KINDS[bad[0][1] // 8])
        same = (c["threshold"] == r.thr_after[lo:lo + n]) | (np.isnan(c["threshold"]) & np.isnan(r.thr_after[lo:lo + n]))
        bad = np.argwhere(~same)
        assert not len(bad), where + ("threshold, first at (slot, ARFCN)", bad[0], rf.KINDS[bad[0][1] // 8], c["threshold"][tuple(bad[0])],
                                      r.thr_after[lo + bad[0][0], bad[0][1]])
        for key in out:
            out[key][lo:lo + n] = c[key]
        if keep_soft:
            softs.append(c["soft"][:, soft_of].copy() if soft_of is not None else c["soft"][c["valid"]])
    final = np.array([g.energy_threshold(a) for a in range(S)])
    bad = np.flatnonzero(final != r.final_thr)
    assert not len(bad), (plan_name, leg, "final thresholds", bad, final[bad], r.final_thr[bad])
    g.close(); ctx.close()
    out["soft"] = np.concatenate(softs) if keep_soft else None
    return out, final


@pytest.mark.parametrize("plan", ["A", "B"])
@pytest.mark.parametrize("leg", [0, 1])
def test_every_form_equals_the_scalar_model(pkg, hip, expected, leg, plan, request):
    """Both TSC legs x both call plans, each under both settings of TRXSIG_TUNE_GROUP_REPLAY (0: the wave form up to 1,024 slots;
    1: the forms that step through every slot): after every call the detectors' flags and avgPwr equal the atoms' oracle values,
    valid and threshold-after equal the scalar model for every ARFCN and slot, and so do the thresholds at the end.  The two
    settings agree on every output, soft bits included -- on the equalising leg (0) that holds k_group_cache_wave to k_group_cache:
    a burst equalised with stale taps, or with the other channel's, has other soft bits."""
    knob = pkg.TrxSig(rf.SPS, 0)
    request.addfinalizer(lambda: (knob.set_tuning(group_replay=0), knob.close()))
    t0 = time.time()
    expected(plan)
    t1 = time.time()
    outs = []
    for form in (0, 1):
        knob.set_tuning(group_replay=form)
        outs.append(run_group(pkg, hip, leg, plan, expected))
    knob.set_tuning(group_replay=0)
    (o0, f0), (o1, f1) = outs
    for key in o0:
        assert np.array_equal(o0[key], o1[key], equal_nan=(key == "threshold")), key
    assert np.array_equal(f0, f1)
    assert o0["valid"].sum() > 100000
    print("leg %d plan %s: schedules %.1f s, two group runs %.1f s" % (leg, plan, t1 - t0, time.time() - t1))


SINGLE = {                                                               # plan -> [(kind, seed, slots)]: what goes through single objects too
    "A": [("a_floor", 3, 900), ("e_negative", 2, None), ("i_cache", 1, None), ("i_cache_V", 1, 4000)],
    "B": [("f_giant", 0, None), ("f_giant", 1, None), ("f_giant", 7, None), ("e_negative", 5, 5000), ("i_cache", 6, 5000)],
}


@pytest.mark.parametrize("plan", ["A", "B"])
def test_single_objects_agree(pkg, hip, expected, plan):
    """A few ARFCNs of the kinds a, e, f and i, a few thousand bursts in all, through independent single-burst objects
    (include/trxsig_transceiver.h: the product's other implementation of pullRadioVector) with the same (tn, fn) sequence: soft bits,
    RSSI, timing offset and threshold equal the group's on the equalising leg.  That ties the scalar model to a second implementation
    and checks WHICH taps equalised each burst (the model only says which burst estimated them).  f_giant's span ends 600 slots
    after its threshold has passed 2^52."""
    r, det, avg = expected(plan)
    p, A = r.plan, rf.atoms()
    cols, upto = [], []
    for kind, seed, n in SINGLE[plan]:
        a = 8 * rf.KINDS.index(kind) + seed
        if kind == "f_giant":
            big = np.flatnonzero(r.thr_state[:, a] >= rf.TWO52)
            assert len(big), "f_giant never went giant in plan %s" % plan
            n = int(big[0]) + 600
        cols.append(a); upto.append(p.n if n is None else min(n, p.n))
    t0 = time.time()
    out, _ = run_group(pkg, hip, pkg.TSCLEG_EQUALIZE, plan, expected, soft_of=cols)
    t1 = time.time()
    bursts = 0
    seen = dict(valid=0, est=0, kept=0, giant=0, negative=0)
    for j, (a, n) in enumerate(zip(cols, upto)):
        o = pkg.TrxHost(rf.SPS, 0, start=p.start, tsc_leg=pkg.TSCLEG_EQUALIZE)
        for cmd in rf.control_commands(a):
            o.control(cmd)
        for t in range(n):
            ai = r.atom[t, a]
            if ai < 0:
                continue
            tn, fn = int(p.tn[t]), int(p.fn[t])
            got = o.pull_radio_vector(A.cells[ai][:157 if tn % 4 == 0 else 156], tn, fn)
            bursts += 1
            where = (plan, rf.KINDS[a // 8], a, t)
            assert o.energy_threshold == out["threshold"][t, a] == r.thr_after[t, a], where + (o.energy_threshold, out["threshold"][t, a], r.thr_after[t, a])
            assert (got is not None) == bool(out["valid"][t, a]), where
            seen["giant"] += r.thr_after[t, a] >= rf.TWO52
            seen["negative"] += r.thr_after[t, a] < 0
            if got is None:
                continue
            assert got[1] == out["rssi"][t, a] and got[2] == out["timing"][t, a], where
            assert np.array_equal(np.asarray(got[0][:148], np.float32), out["soft"][t, j]), where + ("soft bits", int(r.taps[t, a]))
            seen["valid"] += 1
            seen["est"] += bool(r.est[t, a]); seen["kept"] += r.ctype[t, a] == tm.TSC and not r.est[t, a]
        o.close()
    assert bursts <= 8000, bursts
    assert seen["valid"] > 1000 and seen["est"] > 20 and seen["kept"] > 500, seen
    assert (seen["giant"] > 100) if plan == "B" else (seen["negative"] > 20), seen
    print("plan %s: group run %.1f s, %d bursts through single objects %.1f s" % (plan, t1 - t0, bursts, time.time() - t1))
